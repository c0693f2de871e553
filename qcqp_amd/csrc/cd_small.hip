// cd_small_kernel -- improve_coord_descent (qcqp.py:181-192) for a batch of SMALL problems (n <= 64; n <= 128 in the wide kernels below) that share their separable
// constraints and differ in their objective, R restarts each, inside one persistent launch (cd_small.h); in the per-problem-constraint
// mode (cd_small_kernel<MAXC, true>) they share the STRUCTURE of the lists and problem b's coefficients are staged with its objective.
//
// Layout: the ticket frame of small_batch.h around P0_b (n x n doubles, at most 32 KB), workgroups of four waves, LANE = COORDINATE.
//   suggest(RANDOM)   lane j draws the keyed normal (seed_b, first_index + r, j) of qcqpmi_pop_randn;
//   phase 1           every lane visits its own coordinate through p1_sep_visit (cd_phase1_sep.h) -- a sweep is element-wise for
//                     separable constraints --, the sweep's max violation and "any update" are wave reductions; the loop and
//                     its two exits are those of cd_phase1_sep_kernel (kernels_impl.h);
//   gate              max violation of the point (a wave maximum of the lanes' own constraints) < viol_tol, qcqp.py:189;
//   phase 2           the lanes hold x, the OFF-DIAGONAL row sums h_j = sum_{k != j} P0[j][k] x_k and the feasible set of their
//                     coordinate at the slack the phase fixes (compute_set, cd_chain.h).  A visit of coordinate i broadcasts lane
//                     i's values (v_readlane), every lane makes the scalar decision in the reference's arithmetic
//                     (onevar_minimise, onevar.h; chain_commit, cd_chain.h) and an accepted move is a rank-one update along
//                     column i: h_j += P0[i][j] delta.  P0 is symmetric, so column i is read as ROW i of the LDS image -- lane j
//                     reads word i n + j: consecutive doubles, no bank conflict (64 dwords per half-wave);
//   every sweep       h and the objective are recomputed exactly (no drift from one sweep to the next), each sum in ascending
//                     index order: t1 = 2 h_i + q_i and f0 = sum_i (row_i + q_i) x_i + r are the sums the CPU oracle's
//                     improve_cd_sep forms (oracle/qcqp_oracle.c: sep_phase2, quad_eval_skip), term for term;
//   results           objective (the same sum) and max violation of the final point, the counters of qcqpmi_cd_run, the point.
// The scalar decision of a visit is computed by all 64 lanes on the same values: the layout spends lanes to keep the restart's
// state in registers and its matrix in LDS; what runs in parallel are the waves (up to 16 per CU) and phase 1.
//
// WIDE KERNELS (cd_small_kernel<MAXC, pc, 2>, 64 < n <= 128, qcqpmi_cd_batch_run).  The same layout with TWO
// coordinates per lane: lane l holds coordinate l in slot 0 and coordinate l + 64 in slot 1 (live where l + 64 < n); x, h, the diagonal,
// q and the feasible set exist once per slot.  A visit of coordinate i reads slot i >> 6 (wave-uniform) at lane i & 63, its rank-one
// update covers both slots (lane l reads words i n + l and i n + l + 64 of the image); the keyed draws go by the coordinate index; the
// sums of the refresh run over k = 0..n-1 and j = 0..n-1 in ascending order across both slots -- the terms of improve_cd_sep, as before.
// Phase 1 visits both coordinates of a lane, its reductions run over both slots, and status1 is that of the highest coordinate with a
// code.  The image is the same (P0_b n x n, q0_b, [3][m] coefficients, two control words: at most 144 392 bytes, one workgroup per CU from
// n = 101) and the workgroup has up to 512 threads.  With up to four constraints per coordinate the two FeasSet<4> of a lane do not fit
// beside the visit: those kernels recompute coordinate i's set at its visit (same inputs, same code, same bits).  The slots are written
// out (slot 0, then slot 1 under if constexpr) instead of looped over: with loops the W = 1 kernels came out as other code.
#include "cd_small.h"

#include "sm_restart.h"    // the restart: sm_restart<MAXC, PC, W> and its helpers

namespace qcqpmi {
namespace {

// PC: per-problem constraint coefficients (cd_small.h), staged by the frame; the visit arithmetic is the one copy of sm_restart.h.
// W = 2: the wide kernels (64 < n <= 128).  Their workgroup is CD_WIDE_THREADS threads or fewer (the launch decides; blockDim.x).
template <int MAXC, bool PC = false, int W = 1>
__global__ __launch_bounds__(W == 1 ? 256 : CD_WIDE_THREADS) void cd_small_kernel(CdSmallArgs a) {
    extern __shared__ double sm_lds[];
    small_ticket_frame<PC>(
        a, sm_lds, W == 1 ? 256 : (int)blockDim.x,
        [&a](int64_t off, double *Ps, int nn, int tid, int nt) __attribute__((always_inline)) { small_stage_matrix(Ps, a.P0s + off, nn, tid, nt); return nullptr; },
        [&a](const double *Ps, const double *qs, int64_t b, int64_t r, int lane) __attribute__((always_inline)) { sm_restart<MAXC, PC, W>(a, Ps, qs, b, r, lane); });
}

__global__ void small_gather_kernel(const double *__restrict__ X, int64_t n, int64_t R, const int64_t *__restrict__ idx,
                                    double *__restrict__ out) {
    const int64_t b = blockIdx.x, w = idx[2 * b];
    if (w < 0) return;
    for (int64_t j = threadIdx.x; j < n; j += blockDim.x) out[b * n + j] = X[(b * R + w) * n + j];
}

typedef void (*CdSmallKernel)(CdSmallArgs);

CdSmallKernel cd_small_pick(int64_t n, int maxc, bool pc) {
    if (n > CD_SMALL_MAXN) {
        if (pc) return maxc <= 1 ? cd_small_kernel<1, true, 2> : cd_small_kernel<4, true, 2>;
        return maxc <= 1 ? cd_small_kernel<1, false, 2> : cd_small_kernel<4, false, 2>;
    }
    if (pc) return maxc <= 1 ? cd_small_kernel<1, true> : cd_small_kernel<4, true>;
    return maxc <= 1 ? cd_small_kernel<1> : cd_small_kernel<4>;
}

}  // namespace

static int cd_wide_threads_asked() {      // read once
    static const int asked = small_threads_asked("QCQPMI_CD_WIDE_THREADS", CD_WIDE_THREADS);
    return asked;
}

int cd_small_workgroups(int64_t n, int maxc, int64_t pc_entries, int64_t tickets, int device, int *threads) {
    const bool wide = n > CD_SMALL_MAXN;
    return small_ticket_workgroups((const void *)cd_small_pick(n, maxc, pc_entries > 0), small_image_bytes(n, pc_entries), tickets, device,
                                   wide ? CD_WIDE_THREADS : 0, wide ? cd_wide_threads_asked() : 0, threads);
}

int cd_small_launch(const CdSmallArgs &a, int maxc, int wgs, int threads, hipStream_t st) {
    const bool pc = a.cons != nullptr;
    return small_launch(cd_small_pick(a.P.n, maxc, pc), small_image_bytes(a.P.n, pc ? a.P.m : 0), a, wgs, threads, a.P.n > CD_SMALL_MAXN, st);
}

const char *cd_small_name(int maxc, bool pc, bool wide) { return batch_kernel_name<CdSmallArgs>("cd_small_kernel", maxc, pc, wide); }

int small_gather_launch(const double *X, int64_t n, int64_t R, int64_t B, const int64_t *idx, double *out, hipStream_t st) {
    hipLaunchKernelGGL(small_gather_kernel, dim3((unsigned)B), dim3(64), 0, st, X, n, R, idx, out);
    return (int)hipGetLastError();
}

}  // namespace qcqpmi
