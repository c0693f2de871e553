// chain_small_kernel -- a chain of improve methods (COORD_DESCENT, ADMM; up to four stages) for a batch of SMALL problems (n <= 64) inside
// one persistent launch (chain_small.h).
//
// Layout: the chain frame of small_batch.h, workgroups of four waves, LANE = COORDINATE.  A ticket (problem b, a chunk of its restarts)
// is worked through the stages one after the other by ONE workgroup: per stage the image is replaced -- P0_b for a CD stage, Minv_b for
// an ADMM stage (which reads P0_b from global memory, as admm_small_kernel does) -- and every restart of the chunk is run once by
// whichever wave takes it: sm_restart<MAXC, PC, 1> (sm_restart.h) or as_restart<MAXC> (as_restart.h), the bodies of cd_small_kernel and
// admm_small_kernel, handed the argument struct of the single kernel filled from the stage's descriptor.  Stage 0 starts as the single
// kernels do; stage s > 0 runs with generate = 0 and X0 = X: the wave that reads X[o] at the start of its restart is the only writer of
// X[o] in that stage, so the buffer is updated in place.  The hand-over between the stages is the frame's barrier.
#include "chain_small.h"

#include "sm_restart.h"
#include "as_restart.h"

namespace qcqpmi {
namespace {

template <int MAXC, bool PC = false>
__global__ __launch_bounds__(256) void chain_small_kernel(ChainSmallArgs a) {
    extern __shared__ double ch_lds[];
    small_chain_frame<PC>(
        a, ch_lds, 256,
        [&a](int s, int64_t off, double *As, int nn, int tid, int nt) __attribute__((always_inline)) -> const double * {
            const bool admm = a.st[s].method == CHAIN_ADMM;
            small_stage_matrix(As, (admm ? a.Minvs : a.P0s) + off, nn, tid, nt);
            return admm ? a.P0s + off : nullptr;      // the scan covers P0_b too: an ADMM stage reads its columns as rows from global memory
        },
        [&a](int s, const double *As, const double *qs, double *cs, int64_t b, int64_t r, int lane) __attribute__((always_inline)) {
            const ChainStage &g = a.st[s];
            DevProblem P = a.P;
            if constexpr (PC) { P.cp = cs; P.cq = cs + P.m; P.cr = cs + 2 * P.m; }      // the view (small_ticket_frame)
            const int generate = s == 0 ? a.generate : 0;
            const double *X0 = s == 0 ? a.X0 : a.X;
            if (g.method == CHAIN_ADMM) {
                AdmmSmallArgs t;
                t.P = P; t.B = a.B; t.R = a.R; t.RC = a.RC; t.chunks = a.chunks;
                t.P0s = a.P0s; t.q0s = a.q0s; t.r0s = a.r0s; t.rhos = a.rhos; t.Minvs = a.Minvs; t.X0 = X0; t.cons = a.cons;
                t.generate = generate; t.phase1 = g.phase1; t.num_iters = g.num_iters; t.tol = g.tol; t.viol_lim = g.viol_lim;
                t.seed = a.seed; t.seed_stride = a.seed_stride; t.first_index = a.first_index;
                t.ticket = a.ticket;
                t.iters1 = g.iters1; t.iters2 = g.iters2; t.f0 = g.f0; t.maxviol = g.maxviol;
                t.X = a.X;
                as_restart<MAXC>(t, As, qs, b, r, lane);
            } else {
                CdSmallArgs t;
                t.P = P; t.B = a.B; t.R = a.R; t.RC = a.RC; t.chunks = a.chunks;
                t.P0s = a.P0s; t.q0s = a.q0s; t.r0s = a.r0s; t.X0 = X0;
                t.generate = generate; t.phase1 = g.phase1; t.num_iters = g.num_iters; t.viol_tol = g.viol_tol; t.tol = g.tol;
                t.seed = a.seed; t.seed_stride = a.seed_stride; t.first_index = a.first_index;
                t.ticket = a.ticket;
                t.sweeps1 = g.sweeps1; t.sweeps2 = g.sweeps2; t.visits2 = g.visits2; t.accepted2 = g.accepted2;
                t.ran2 = g.ran2; t.status1 = g.status1; t.status2 = g.status2; t.f0 = g.f0; t.maxviol = g.maxviol;
                t.X = a.X;
                t.cons = a.cons;
                sm_restart<MAXC, PC, 1>(t, As, qs, b, r, lane);
            }
        });
}

typedef void (*ChainSmallKernel)(ChainSmallArgs);

ChainSmallKernel chain_small_pick(int maxc, bool pc) {
    if (pc) return maxc <= 1 ? chain_small_kernel<1, true> : chain_small_kernel<4, true>;
    return maxc <= 1 ? chain_small_kernel<1> : chain_small_kernel<4>;
}

}  // namespace

int chain_small_workgroups(int64_t n, int maxc, int64_t pc_entries, int64_t tickets, int device) {
    int per = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, chain_small_pick(maxc, pc_entries > 0), 256, small_image_bytes(n, pc_entries));
    if (e != hipSuccess) return -(int)e;
    return small_workgroup_cap(device, per, tickets);
}

int chain_small_launch(const ChainSmallArgs &a, int maxc, int wgs, hipStream_t st) {
    const bool pc = a.cons != nullptr;
    return small_launch(chain_small_pick(maxc, pc), small_image_bytes(a.P.n, pc ? a.P.m : 0), a, wgs, 256, false, st);
}

const char *chain_small_name(int maxc, bool pc) { return batch_kernel_name<ChainSmallArgs>("chain_small_kernel", maxc, pc, false); }

}  // namespace qcqpmi
