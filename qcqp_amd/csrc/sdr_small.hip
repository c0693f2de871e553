// sdr_small_kernel -- suggest(SDR) for a batch of SMALL problems (n <= 64) of the unit-diagonal family that differ in their
// objective: relaxation by the mixing method, multipliers and samples of every problem inside one persistent launch (sdr_small.h).
//
// Layout.  ONE WAVEFRONT PER PROBLEM, one wavefront per workgroup: a wave draws a problem from a global counter (an ordinary atomic
// add), builds C_b (N x N doubles) in its LDS from P0_b, q0_b, r0_b and s = sqrt(d) (the shared one, or problem b's row of a [B][n] array), keeps V_b (N rows of 64, row stride 65
// doubles) beside it and never waits for another wave: no flags, no spinning; the barriers below are those of a one-wave workgroup
// and order the wave's own LDS traffic where lanes read what other lanes wrote.
//   sweeps      LANE = COMPONENT k of V.  g_i[k] = sum_{j != i} C_ij V[j][k]: C_ij is one address for the whole wave (a broadcast
//               read), V[j][lane] consecutive doubles (no bank conflict); ||g_i||^2 and v_i . g_i are wave sums in the fixed order of
//               wave_sum_tree (dev_util.h).  The passes are those of sdr_mixing_kernel (sdr_solve.h): objective, sweeps until
//               |delta_sweep| <= tol (1 + |f|) or max_sweeps, objective again; a row with ||g_i|| = 0 stays as it is (MAXCUT's
//               homogenising row: q0 = 0);
//   multipliers the last pass forms y_i = -(v_i . g_i + C_ii v_i . v_i) = -v_i . (C v)_i; the objective is the sum of the same terms;
//   samples     LANE = COORDINATE i.  u = v_n; lane k draws xi_k and forms w_k = xi_k - u_k (u . xi), the wave leaves w in LDS and
//               lane i forms x_i = s_i (v_i . u + v_i . w), both sums over k in ascending order: V[i][k] at row stride 65 puts the 32
//               lanes of a half-wave on 32 different bank pairs, w_k is a broadcast read.
// LDS per wave: (65 N + N^2 + 64) doubles -- 26.4 KB at n = 32 (six waves per CU), 68.1 KB at n = 64 (two).
// sdr_small_kernel<true> (65 <= n <= 128) is the same wave with C_b PACKED (the lower triangle, N (N + 1) / 2 doubles: 134 672 bytes of
// LDS at n = 128, one wave per CU) and TWO coordinates per lane in the samples (lane l: x_l and x_{l+64}); sdr_small.h has the details.
#include "sdr_small.h"

#include "philox.h"
#include "dev_util.h"
#include "small_batch.h"    // the launchers: small_wave_workgroups, small_launch

namespace qcqpmi {
namespace {

// g (lane k) = sum_{j != i} C_ij V[j][k]: four partial sums over j = 0, 1, 2, 3 (mod 4) in ascending j -- what is left of N after
// the last full four goes to the first --, combined as (a0 + a1) + (a2 + a3)
__device__ inline double ss_row_product(const double *Cs, const double *Vs, int N, int i, int lane) {
    const double *Ci = Cs + i * N, *Vl = Vs + lane;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int j = 0;
    for (; j + 4 <= N; j += 4) {
        const double c0 = (j == i) ? 0.0 : Ci[j], c1 = (j + 1 == i) ? 0.0 : Ci[j + 1];
        const double c2 = (j + 2 == i) ? 0.0 : Ci[j + 2], c3 = (j + 3 == i) ? 0.0 : Ci[j + 3];
        a0 = __builtin_fma(c0, Vl[j * SDR_SMALL_VSTR], a0);
        a1 = __builtin_fma(c1, Vl[(j + 1) * SDR_SMALL_VSTR], a1);
        a2 = __builtin_fma(c2, Vl[(j + 2) * SDR_SMALL_VSTR], a2);
        a3 = __builtin_fma(c3, Vl[(j + 3) * SDR_SMALL_VSTR], a3);
    }
    for (; j < N; j++) a0 = __builtin_fma((j == i) ? 0.0 : Ci[j], Vl[j * SDR_SMALL_VSTR], a0);
    return (a0 + a1) + (a2 + a3);
}

// C_b packed (the wide kernel): the lower triangle with the diagonal, row after row -- C_ij at tri(max(i, j)) + min(i, j)
__device__ inline int ss_tri(int i) { return i * (i + 1) / 2; }
__device__ inline double ss_packed(const double *Cs, int i, int j) { return Cs[j < i ? ss_tri(i) + j : ss_tri(j) + i]; }

// the same sum in the same association from the packed image: only the address of C_ij differs (wave-uniform: a broadcast read)
__device__ inline double ss_row_product_packed(const double *Cs, const double *Vs, int N, int i, int lane) {
    const double *Vl = Vs + lane;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int j = 0;
    for (; j + 4 <= N; j += 4) {
        const double c0 = (j == i) ? 0.0 : ss_packed(Cs, i, j), c1 = (j + 1 == i) ? 0.0 : ss_packed(Cs, i, j + 1);
        const double c2 = (j + 2 == i) ? 0.0 : ss_packed(Cs, i, j + 2), c3 = (j + 3 == i) ? 0.0 : ss_packed(Cs, i, j + 3);
        a0 = __builtin_fma(c0, Vl[j * SDR_SMALL_VSTR], a0);
        a1 = __builtin_fma(c1, Vl[(j + 1) * SDR_SMALL_VSTR], a1);
        a2 = __builtin_fma(c2, Vl[(j + 2) * SDR_SMALL_VSTR], a2);
        a3 = __builtin_fma(c3, Vl[(j + 3) * SDR_SMALL_VSTR], a3);
    }
    for (; j < N; j++) a0 = __builtin_fma((j == i) ? 0.0 : ss_packed(Cs, i, j), Vl[j * SDR_SMALL_VSTR], a0);
    return (a0 + a1) + (a2 + a3);
}

// W2 (the wide kernel, 65 <= n <= 128): C_b packed, two coordinates per lane in the samples
template <bool W2>
__device__ inline void ss_problem(const SdrSmallArgs &a, double *Vs, double *Cs, double *ws, int64_t b, int lane) {
    const int n = a.n, N = n + 1;
    const uint64_t seed = a.seed + (uint64_t)b * a.seed_stride;
    __syncthreads();             // the wave is done with the LDS image of its previous problem

    // ---- C_b (sdr.lifted_cost, the same products); a matrix that is not symmetric (or holds a NaN) makes the call fail
    const double *Pg = a.P0s + b * n * n, *qg = a.q0s + b * n, *sv = a.s + b * a.s_stride;
    bool asym = false;
    if constexpr (W2) {
        // row i of the triangle, lane = column j <= i: every pair (i, j) is compared once, the diagonal with itself (a NaN)
        for (int i = 0; i < N; i++) {
            double *Ci = Cs + ss_tri(i);
            for (int j = lane; j <= i; j += 64) {
                double c;
                if (i < n) {
                    const double p = Pg[i * n + j];
                    asym = asym || !(p == Pg[j * n + i]);
                    c = p * (sv[i] * sv[j]);
                } else if (j < n) {
                    c = 0.5 * qg[j] * sv[j];
                } else {
                    c = a.r0s[b];
                }
                Ci[j] = c;
            }
        }
    } else
    for (int e = lane; e < N * N; e += 64) {
        const int i = e / N, j = e - i * N;
        double c;
        if (i < n && j < n) {
            const double p = Pg[i * n + j];
            asym = asym || (j > i && !(p == Pg[j * n + i]));
            c = p * (sv[i] * sv[j]);
        } else if (i < n) {
            c = 0.5 * qg[i] * sv[i];
        } else if (j < n) {
            c = 0.5 * qg[j] * sv[j];
        } else {
            c = a.r0s[b];
        }
        Cs[e] = c;
    }
    if (asym) a.ticket[1] = 1;

    // ---- the start (sdr_small.h): keyed normal rows, normalised; or the caller's
    for (int i = 0; i < N; i++) {
        double v;
        if (a.V0s) {
            v = a.V0s[(b * N + i) * SDR_SMALL_K + lane];
        } else {
            const double z = keyed_normal(seed, ~0ull - (uint64_t)i, (uint64_t)lane);
            v = z / sqrt(wave_sum_tree(z * z));
        }
        Vs[i * SDR_SMALL_VSTR + lane] = v;
    }
    __syncthreads();

    // ---- pass -1: objective only; passes 0..: sweeps; last pass: objective and multipliers (the passes of sdr_mixing_kernel)
    double f = 0.0;
    int sweeps = 0;
    for (int pass = -1; pass <= a.max_sweeps; pass++) {
        const bool update = pass >= 0 && pass < a.max_sweeps;
        double facc = 0.0, dsweep = 0.0;
        for (int i = 0; i < N; i++) {
            double g;
            if constexpr (W2) g = ss_row_product_packed(Cs, Vs, N, i, lane);
            else g = ss_row_product(Cs, Vs, N, i, lane);
            const double vold = Vs[i * SDR_SMALL_VSTR + lane];
            const double gv = wave_sum_tree(g * vold);
            if (update) {
                const double nrm = sqrt(wave_sum_tree(g * g));
                if (nrm > 0.0) {
                    Vs[i * SDR_SMALL_VSTR + lane] = -g / nrm;
                    dsweep += -2.0 * (nrm + gv);      // exact change of <C, V V^T>
                }
            } else {
                const double t = gv + Cs[W2 ? ss_tri(i) + i : i * N + i] * wave_sum_tree(vold * vold);      // v_i . (C v)_i
                facc += t;
                if (pass >= 0 && lane == 0) a.y[b * N + i] = -t;
            }
        }
        bool conv = false;
        if (!update) {
            f = facc;
        } else {
            f += dsweep;
            sweeps++;
            conv = fabs(dsweep) <= a.tol * (1.0 + fabs(f));
        }
        if (pass == a.max_sweeps) break;
        if (conv) pass = a.max_sweeps - 1;      // converged: jump to the last pass
    }
    for (int i = 0; i < N; i++) a.V[(b * N + i) * SDR_SMALL_K + lane] = Vs[i * SDR_SMALL_VSTR + lane];
    if (lane == 0) { a.primal[b] = f; a.sweeps[b] = sweeps; }
    __syncthreads();             // the rows were written with lane = component; the samples read them with lane = coordinate

    // ---- samples: x = s o (V_n u + V_n (xi - u (u . xi)))
    if (a.S > 0) {
        const int il = lane < n ? lane : 0;
        const double *Vi = Vs + il * SDR_SMALL_VSTR, *U = Vs + n * SDR_SMALL_VSTR;
        const double u = U[lane], si = sv[il];
        double mu = 0.0;
        for (int k = 0; k < SDR_SMALL_K; k++) mu = __builtin_fma(Vi[k], U[k], mu);
        // the wide kernel's slot 1: lane l also forms coordinate l + 64 (live where l + 64 < n), the same sums from the same U and w
        const bool on1 = W2 && lane + 64 < n;
        const double *Vi1 = Vs + (on1 ? lane + 64 : 0) * SDR_SMALL_VSTR;
        double mu1 = 0.0, si1 = 0.0;
        if constexpr (W2) {
            for (int k = 0; k < SDR_SMALL_K; k++) mu1 = __builtin_fma(Vi1[k], U[k], mu1);
            if (on1) si1 = sv[lane + 64];
        }
        for (int64_t sg = 0; sg < a.S; sg++) {
            const double xi = keyed_normal(seed, a.first_index + (uint64_t)sg, (uint64_t)lane);
            const double w = xi - u * wave_sum_tree(u * xi);
            __syncthreads();     // every lane has read the previous sample's w
            ws[lane] = w;
            __syncthreads();
            double t = 0.0;
            for (int k = 0; k < SDR_SMALL_K; k++) t = __builtin_fma(Vi[k], ws[k], t);
            if (lane < n) a.X[(b * a.S + sg) * n + lane] = si * (mu + t);
            if constexpr (W2) {
                double t1 = 0.0;
                for (int k = 0; k < SDR_SMALL_K; k++) t1 = __builtin_fma(Vi1[k], ws[k], t1);
                if (on1) a.X[(b * a.S + sg) * n + lane + 64] = si1 * (mu1 + t1);
            }
        }
    }
}

template <bool W2>
__global__ __launch_bounds__(64) void sdr_small_kernel(SdrSmallArgs a) {
    extern __shared__ __attribute__((aligned(16))) double ss_lds[];
    const int N = a.n + 1, lane = threadIdx.x;
    double *Vs = ss_lds, *Cs = Vs + N * SDR_SMALL_VSTR, *ws = Cs + (W2 ? N * (N + 1) / 2 : N * N);
    for (;;) {
        int tk = 0;
        if (lane == 0) tk = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tk = __builtin_amdgcn_readfirstlane(tk);
        if (tk >= a.B) break;
        ss_problem<W2>(a, Vs, Cs, ws, tk, lane);
    }
}

typedef void (*SdrSmallKernel)(SdrSmallArgs);

// n <= SDR_SMALL_MAXN: the kernel with the full C_b; past it the wide one
SdrSmallKernel ss_kernel(int n) { return n > SDR_SMALL_MAXN ? sdr_small_kernel<true> : sdr_small_kernel<false>; }

}  // namespace

size_t sdr_small_lds_bytes(int n) {
    const size_t N = (size_t)n + 1;
    return (N * SDR_SMALL_VSTR + (n > SDR_SMALL_MAXN ? N * (N + 1) / 2 : N * N) + SDR_SMALL_K) * sizeof(double);
}

int sdr_small_workgroups(int n, int64_t B, int device) { return small_wave_workgroups((const void *)ss_kernel(n), sdr_small_lds_bytes(n), B, device); }

int sdr_small_launch(const SdrSmallArgs &a, int wgs, hipStream_t st) { return small_launch(ss_kernel(a.n), sdr_small_lds_bytes(a.n), a, wgs, 64, true, st); }

}  // namespace qcqpmi
