// cd_small_kernel -- improve_coord_descent (qcqp.py:181-192) for a batch of SMALL problems (n <= 64) that share their separable
// constraints and differ in their objective, R restarts each, inside one persistent launch (cd_small.h); in the per-problem-constraint
// mode (cd_small_kernel<MAXC, true>) they share the STRUCTURE of the lists and problem b's coefficients are staged with its objective.
//
// Layout.  ONE WAVEFRONT PER (problem, restart), LANE = COORDINATE.  A workgroup of four waves draws a ticket -- a problem and a
// chunk of its restarts -- from a global counter (an ordinary atomic add), stages P0_b (n x n doubles, at most 32 KB) and q0_b in
// LDS once, and its waves take the chunk's restarts one by one from a counter in LDS.  After the barrier that follows the staging
// a wave never waits for another one: no flags, no spinning; the next barrier is the one before the LDS image is replaced.
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
#include "cd_small.h"

#include "onevar.h"
#include "cd_phase1_sep.h"
#include "cd_chain.h"      // compute_set, ChainState, chain_commit, readlane_d
#include "dev_util.h"

namespace qcqpmi {
namespace {

// max violation of coordinate i's own constraints at xi (the expression of eval_kernel; -inf without a constraint)
__device__ inline double sm_coord_viol(const DevProblem &P, int i, double xi) {
    double v = -QM_INF;
    for (int e = P.cptr[i]; e < P.cptr[i + 1]; e++) {
        const double w = viol_of((P.cp[e] * xi + P.cq[e]) * xi + P.cr[e], P.crel[e]);
        v = w > v ? w : v;
    }
    return v;
}

// h (lane j) = sum_{k != j} P0[k][j] x_k in ascending k; returns f0(x) = sum_j (row_j + q_j) x_j + r0 in ascending j, row_j the
// same sum with the diagonal term.  x is zero in the lanes >= n.
__device__ inline double sm_refresh(const double *Ps, const double *qs, double r0, int n, int lane, double x, double &h) {
    const int lc = lane < n ? lane : 0;
    double row = 0.0;
    h = 0.0;
    for (int k = 0; k < n; k++) {
        const double prod = Ps[k * n + lc] * readlane_d(x, k);
        row += prod;
        h = (k == lane) ? h : h + prod;
    }
    const double term = (row + qs[lc]) * x;
    double acc = 0.0;
    for (int k = 0; k < n; k++) acc += readlane_d(term, k);
    return acc + r0;
}

// a.P: the constraint lists the restart reads -- the context's, or the view of problem b's staged coefficients (cd_small_kernel).
// PC only names the caller: every kernel keeps an instance of its own, inlined as the single-caller function it was.
template <int MAXC, bool PC>
__device__ inline void sm_restart(const CdSmallArgs &a, const double *Ps, const double *qs, int64_t b, int64_t r, int lane) {
    const DevProblem &P = a.P;
    const int n = (int)P.n;
    const bool on = lane < n;
    const int lc = on ? lane : 0;
    const uint64_t seed = a.seed + (uint64_t)b * a.seed_stride;
    const uint64_t gr = a.first_index + (uint64_t)r;
    const int64_t o = b * a.R + r;
    const double r0 = a.r0s[b];
    double x = 0.0;
    if (on) x = a.generate ? keyed_normal(seed, gr, (uint64_t)lane) : a.X0[o * n + lane];

    // ---- phase 1 (qcqp.py:101-149): the loop of cd_phase1_sep_kernel for one restart, a coordinate per lane
    int64_t sweeps1 = 0;
    int st1 = 0;
    if (a.phase1) {
        int my_status = 0;
        bool fin = false;
        for (int64_t t = 0; t < a.num_iters && !fin; t++) {
            sweeps1++;
            double vmax = -QM_INF;
            bool upd = false;
            if (on) {
                double xi = x;
                P1Visit V;
                p1_sep_visit<MAXC>(P, lane, xi, a.tol, a.viol_tol, seed, gr, t, V);
                if (V.status) my_status = V.status;
                if (V.visited) {
                    if (V.moved) { x = xi; upd = true; }
                    vmax = V.vafter;
                }
            }
            const double v = wave_max(vmax);
            const bool u = __builtin_amdgcn_ballot_w64(upd) != 0ull;
            // done when feasible enough (qcqp.py:111); a sweep without an update is a fixed point
            fin = v < a.viol_tol || !u;
        }
        const unsigned long long bad = __builtin_amdgcn_ballot_w64(my_status != 0);
        if (bad) st1 = __builtin_amdgcn_readlane(my_status, 63 - __builtin_clzll(bad));      // the highest coordinate's, like the serial kernel
    }

    // ---- gate (qcqp.py:189); the max violation is also the slack phase 2 fixes (qcqp.py:157)
    const double slack = wave_max(on ? sm_coord_viol(P, lane, x) : -QM_INF);
    const bool ran2 = st1 == 0 && slack < a.viol_tol;

    // ---- phase 2 (qcqp.py:152-178)
    ChainState S;
    S.fcur = 0.0; S.upd_counter = 0; S.visits = 0; S.accepted = 0; S.sweeps = 0; S.conv = !ran2; S.status = 0;
    if (ran2) {
        FeasSet<MAXC> Cm;
        Cm.n = 0;
#pragma unroll
        for (int j = 0; j <= MAXC; j++) { Cm.lo[j] = 0.0; Cm.hi[j] = 0.0; }
        if (on) compute_set<MAXC>(P, lane, slack, Cm);
        const double dg = Ps[lc * n + lc], ql = qs[lc];
        for (int64_t t = 0; t < a.num_iters && !S.conv; t++) {
            S.sweeps++;
            double h;
            S.fcur = sm_refresh(Ps, qs, r0, n, lane, x, h);
            for (int i = 0; i < n; i++) {
                const double xi = readlane_d(x, i), t2 = readlane_d(dg, i);
                const double t1 = 2.0 * readlane_d(h, i) + readlane_d(ql, i);
                const double t0 = S.fcur - xi * (t2 * xi + t1);
                FeasSet<MAXC> C;
                C.n = __builtin_amdgcn_readlane(Cm.n, i);
#pragma unroll
                for (int j = 0; j <= MAXC; j++) { C.lo[j] = readlane_d(Cm.lo[j], i); C.hi[j] = readlane_d(Cm.hi[j], i); }
                DrawKey dk{seed, gr, (uint32_t)i, (uint32_t)t | 0x80000000u, 0u};
                double xn = xi;
                const int got = onevar_minimise<MAXC>(t2, t1, t0, C, dk, &xn);
                bool moved;
                double delta;
                chain_commit<MAXC>(S, got, xn, xi, t2, t1, t0, a.tol, n, moved, delta);
                if (moved) {      // rank-one update along column i (= row i of the symmetric image)
                    const double pij = Ps[i * n + lc];
                    h = (lane == i) ? h : h + pij * delta;
                    x = (lane == i) ? xn : x;
                }
                if (S.conv) break;
            }
        }
    }

    // ---- results: objective and max violation of the final point; a restart on which the reference raises never wins
    double hh;
    double f = sm_refresh(Ps, qs, r0, n, lane, x, hh);
    double mv = wave_max(on ? sm_coord_viol(P, lane, x) : -QM_INF);
    if (st1 != 0 || S.status != 0) { f = QM_INF; mv = QM_INF; }
    if (lane == 0) {
        a.sweeps1[o] = sweeps1; a.sweeps2[o] = S.sweeps; a.visits2[o] = S.visits; a.accepted2[o] = S.accepted;
        a.ran2[o] = ran2 ? 1 : 0;
        a.status1[o] = st1; a.status2[o] = S.status;
        a.f0[o] = f; a.maxviol[o] = mv;
    }
    if (on) a.X[o * n + lane] = x;
}

// PC: per-problem constraint coefficients (cd_small.h).  The ticket's workgroup stages problem b's (p, q, r) of every list entry in
// LDS beside P0_b and q0_b -- entry e of the context's lists (cptr order) is constraint cidx[e] of a.cons [B][m][3] -- and its waves
// read their lists through the kernel's copy of the context's DevProblem, whose cp / cq / cr point at that image: cptr and crel stay
// the context's, and the visit arithmetic is the one copy above.
template <int MAXC, bool PC = false>
__global__ __launch_bounds__(256) void cd_small_kernel(CdSmallArgs a) {
    extern __shared__ double sm_lds[];
    const int n = (int)a.P.n, m = PC ? (int)a.P.m : 0;
    double *Ps = sm_lds, *qs = sm_lds + n * n;
    double *cs = qs + n;             // PC: [3][m] the staged coefficients, p then q then r
    int *ctl = (int *)(cs + 3 * m);  // [0] the workgroup's ticket, [1] next restart of its chunk
    const int *cidx = a.P.cidx;
    if constexpr (PC) { a.P.cp = cs; a.P.cq = cs + m; a.P.cr = cs + 2 * m; }      // the view: cptr and crel stay the context's
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t tickets = a.B * a.chunks;
    for (;;) {
        __syncthreads();             // every wave is done with the LDS image of the previous ticket
        if (tid == 0) {
            ctl[0] = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ctl[1] = 0;
        }
        __syncthreads();
        const int64_t tk = ctl[0];
        if (tk >= tickets) break;
        const int64_t b = tk / a.chunks, r_lo = (tk % a.chunks) * a.RC;
        const int64_t r_hi = r_lo + a.RC < a.R ? r_lo + a.RC : a.R;
        const double *Pg = a.P0s + b * n * n;
        for (int e = tid; e < n * n; e += 256) Ps[e] = Pg[e];
        if (tid < n) qs[tid] = a.q0s[b * n + tid];
        if constexpr (PC) {
            const double *cg = a.cons + b * m * 3;
            for (int e = tid; e < m; e += 256) {
                const double *ck = cg + (cidx[e] - 1) * 3;
                cs[e] = ck[0]; cs[m + e] = ck[1]; cs[2 * m + e] = ck[2];
            }
        }
        __syncthreads();
        // the visits read column i as row i: a matrix that is not symmetric (or holds a NaN) makes the call fail
        bool asym = false;
        for (int e = tid; e < n * n; e += 256) {
            const int i = e / n, j = e - i * n;
            asym = asym || (j > i && !(Ps[e] == Ps[j * n + i]));
        }
        if (asym) a.ticket[1] = 1;
        for (;;) {
            int k = 0;
            if (lane == 0) k = atomicAdd(&ctl[1], 1);
            k = __builtin_amdgcn_readfirstlane(k);
            if (r_lo + k >= r_hi) break;
            sm_restart<MAXC, PC>(a, Ps, qs, b, r_lo + k, lane);
        }
    }
}

__global__ void cd_small_gather_kernel(const double *__restrict__ X, int64_t n, int64_t R, const int64_t *__restrict__ idx,
                                       double *__restrict__ out) {
    const int64_t b = blockIdx.x, w = idx[2 * b];
    if (w < 0) return;
    for (int64_t j = threadIdx.x; j < n; j += blockDim.x) out[b * n + j] = X[(b * R + w) * n + j];
}

}  // namespace

size_t cd_small_lds_bytes(int64_t n, int64_t pc_entries) { return (size_t)(n * n + n + 3 * pc_entries) * sizeof(double) + 2 * sizeof(int); }

int cd_small_workgroups(int64_t n, int maxc, int64_t pc_entries, int64_t tickets, int device) {
    int cus = 0, per = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return -(int)e;
    const size_t lds = cd_small_lds_bytes(n, pc_entries);
    if (pc_entries > 0)
        e = (maxc <= 1) ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, cd_small_kernel<1, true>, 256, lds)
                        : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, cd_small_kernel<4, true>, 256, lds);
    else
        e = (maxc <= 1) ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, cd_small_kernel<1>, 256, lds)
                        : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, cd_small_kernel<4>, 256, lds);
    if (e != hipSuccess) return -(int)e;
    if (per < 1) per = 1;
    const int64_t cap = (int64_t)cus * per;
    return (int)(tickets < cap ? tickets : cap);
}

int cd_small_launch(const CdSmallArgs &a, int maxc, int wgs, hipStream_t st) {
    const bool pc = a.cons != nullptr;
    const size_t lds = cd_small_lds_bytes(a.P.n, pc ? a.P.m : 0);
    if (pc && maxc <= 1) hipLaunchKernelGGL((cd_small_kernel<1, true>), dim3((unsigned)wgs), dim3(256), lds, st, a);
    else if (pc) hipLaunchKernelGGL((cd_small_kernel<4, true>), dim3((unsigned)wgs), dim3(256), lds, st, a);
    else if (maxc <= 1) hipLaunchKernelGGL(cd_small_kernel<1>, dim3((unsigned)wgs), dim3(256), lds, st, a);
    else hipLaunchKernelGGL(cd_small_kernel<4>, dim3((unsigned)wgs), dim3(256), lds, st, a);
    return (int)hipGetLastError();
}

const char *cd_small_name(int maxc, bool pc) {
    if (pc) return maxc <= 1 ? "cd_small_kernel<1,pc>" : "cd_small_kernel<4,pc>";
    return maxc <= 1 ? "cd_small_kernel<1>" : "cd_small_kernel<4>";
}

int cd_small_gather_launch(const double *X, int64_t n, int64_t R, int64_t B, const int64_t *idx, double *out, hipStream_t st) {
    hipLaunchKernelGGL(cd_small_gather_kernel, dim3((unsigned)B), dim3(64), 0, st, X, n, R, idx, out);
    return (int)hipGetLastError();
}

}  // namespace qcqpmi
