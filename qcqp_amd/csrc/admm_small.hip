// admm_small_kernel -- improve_admm (qcqp.py:254-285) for a batch of SMALL problems (n <= 64) with separable constraints, R restarts
// each, inside one persistent launch (admm_small.h).
//
// Layout: the ticket frame of small_batch.h around Minv_b = (2 (P0_b + rho_b m I))^-1 (n x n doubles, at most 32 KB), workgroups of
// four waves, LANE = COORDINATE.
//   consensus state   separable constraints move one coordinate each, so the copies x_k and duals u_k of the reference collapse to what
//                     admm_unit_step_kernel keeps: per lane z_i, one dual per constraint on the coordinate (registers) and the sum
//                     S_i of the operands 2 xhat - vhat - z of its constraints; the consensus sum is m z + S;
//   projection        a lane walks the constraints on its coordinate in ascending entry order through admm_small_solve<1> (admm_solve.h: the
//                     one copy of the reference's bracket doubling and bisection, with the one-row shortcut); the bracket of an entry
//                     is what qcqpmi_admm_set_basis derives for one row: slo = -1 / p for p > 0, ehi = -1 / p for p < 0;
//   phase 1           orc_admm_phase1: max violation of z (a wave maximum) < tol ends it, else z = (S + m z) / m and the projections;
//   phase 2           orc_admm_phase2: rhs = 2 rho (S + m z) - q0, z_j = sum_k Minv[k][j] rhs_k in ascending k (rhs_k broadcast by
//                     v_readlane; Minv is symmetric, so column j is read as word k n + j of the image: consecutive doubles), the
//                     projections, |last_z - z| through wave_sum_tree, the exits `< tol` and `maxviol > viol_lim`, and bestx =
//                     better(z, bestx) with f0(z) = z . (rhs / 2 - rho m z + q0) + r0 from the solve itself (admm_take_z_kernel);
//   P0_b              is read from GLOBAL memory, for the objective of the points no solve produced (the start, the phase-1 result)
//                     and of the best point, which is reported through P0 itself like qcqpmi_admm_run does: two or three products per
//                     restart against up to 2 num_iters solves -- the image stays at 32 KB + lists and four workgroups share a CU.
// The wide kernels <MAXC, pc, 2> (64 < n <= 128) keep TWO coordinates per lane -- l and l + 64 --, the same image (up to
// 132 104 bytes + lists) and workgroups of four or eight waves; what changes is spelled out at as_restart.
#include "admm_small.h"

#include "as_restart.h"    // the restarts: as_restart<MAXC>, as_restart_w2<MAXC> and their helpers

namespace qcqpmi {
namespace {

// PC: per-problem constraint coefficients, staged by the frame (small_batch.h)
// W = 2: the wide kernels (64 < n <= 128).  Their workgroup is ADMM_WIDE_THREADS threads or fewer (the launch decides; blockDim.x).
template <int MAXC, bool PC = false, int W = 1>
__global__ __launch_bounds__(W == 1 ? 256 : ADMM_WIDE_THREADS) void admm_small_kernel(AdmmSmallArgs a) {
    extern __shared__ double as_lds[];
    small_ticket_frame<PC>(      // the scan covers P0_b too: its columns are read as rows from global memory
        a, as_lds, W == 1 ? 256 : (int)blockDim.x,
        [&a](int64_t off, double *Ms, int nn, int tid, int nt) __attribute__((always_inline)) {
            const double *Mg = a.Minvs + off, *Pg = a.P0s + off;
            small_stage_matrix(Ms, Mg, nn, tid, nt);
            return Pg;
        },
        [&a](const double *Ms, const double *qs, int64_t b, int64_t r, int lane) __attribute__((always_inline)) {
            if constexpr (W == 2) as_restart_w2<MAXC>(a, Ms, qs, b, r, lane);
            else as_restart<MAXC>(a, Ms, qs, b, r, lane);
        });
}

typedef void (*AdmmSmallKernel)(AdmmSmallArgs);

AdmmSmallKernel admm_small_pick(int64_t n, int maxc, bool pc) {
    if (n > ADMM_SMALL_MAXN) {
        if (pc) return maxc <= 1 ? admm_small_kernel<1, true, 2> : admm_small_kernel<4, true, 2>;
        return maxc <= 1 ? admm_small_kernel<1, false, 2> : admm_small_kernel<4, false, 2>;
    }
    if (pc) return maxc <= 1 ? admm_small_kernel<1, true> : admm_small_kernel<4, true>;
    return maxc <= 1 ? admm_small_kernel<1> : admm_small_kernel<4>;
}

}  // namespace

static int admm_wide_threads_asked() {      // read once
    static const int asked = small_threads_asked("QCQPMI_ADMM_WIDE_THREADS", ADMM_WIDE_THREADS);
    return asked;
}

int admm_small_workgroups(int64_t n, int maxc, int64_t pc_entries, int64_t tickets, int device, int *threads) {
    const bool wide = n > ADMM_SMALL_MAXN;
    return small_ticket_workgroups((const void *)admm_small_pick(n, maxc, pc_entries > 0), small_image_bytes(n, pc_entries), tickets, device,
                                   wide ? ADMM_WIDE_THREADS : 0, wide ? admm_wide_threads_asked() : 0, threads);
}

int admm_small_launch(const AdmmSmallArgs &a, int maxc, int wgs, int threads, hipStream_t st) {
    const bool pc = a.cons != nullptr;
    return small_launch(admm_small_pick(a.P.n, maxc, pc), small_image_bytes(a.P.n, pc ? a.P.m : 0), a, wgs, threads, a.P.n > ADMM_SMALL_MAXN, st);
}

const char *admm_small_name(int maxc, bool pc, bool wide) { return batch_kernel_name<AdmmSmallArgs>("admm_small_kernel", maxc, pc, wide); }

}  // namespace qcqpmi
