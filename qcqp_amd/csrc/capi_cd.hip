// C ABI of libqcqp_mi.so, coordinate descent on the resident population: qcqpmi_cd_run / qcqpmi_cd_run_stage and the switches
// and readers that go with them.  The unit that compiles the phase-1 kernel, the three phase-2 families launch_cd chooses among
// (cd_phase2.h, cd_phase2_rs.h, cd_phase2_q.h), the kernel for coupled constraints (cd_general.h) and the gate between the
// phases; the slot-queue kernel is cd_queue.hip's, the dense-constraint path capi_dense.hip's.  Also what the other runs need
// after their kernels: the per-restart results -> host and the status policy on them (capi_stream.hip, capi_dense.hip).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "capi_ctx.h"
#include "cd_kernels.h"
#include "cd_phase2.h"
#include "cd_phase2_rs.h"
#include "cd_phase2_q.h"
#include "cd_general.h"
#include "cd_queue.h"

using namespace qcqpmi;

namespace {

// per-restart results of a coordinate-descent run -> host: one pack kernel, one copy into pinned memory,
// one synchronisation (nine pageable copies cost ~0.3 ms of staging kernels per call)
__global__ void pack_cd_outputs_kernel(char *out, int64_t R, const int64_t *s1, const int64_t *s2, const int64_t *vis,
                                       const int64_t *acc, const double *f0, const double *mv, const int *st,
                                       const int *st1, const uint8_t *flag) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    int64_t *o64 = (int64_t *)out;
    o64[r] = s1[r]; o64[R + r] = s2[r]; o64[2 * R + r] = vis[r]; o64[3 * R + r] = acc[r];
    double *od = (double *)(out + 32 * R);
    od[r] = f0[r]; od[R + r] = mv[r];
    int *oi = (int *)(out + 48 * R);
    oi[r] = st[r]; oi[R + r] = st1[r];
    ((uint8_t *)(out + 56 * R))[r] = flag[r];
}

}  // namespace

namespace qcqpmi {

// staging buffers (device + pinned host) of fetch_cd_outputs for R restarts
int cd_outputs_reserve(qcqpmi_ctx *c, int64_t R) {
    HIPCHK(c, c->d_out.reserve(c->stream, (size_t)(57 * R), false));
    HIPCHK(c, c->h_out.reserve(c->stream, (size_t)(57 * R), false));
    return 0;
}

int fetch_cd_outputs(qcqpmi_ctx *c, int64_t *sweeps1, int64_t *sweeps2, int64_t *visits2, int64_t *accepted2,
                     uint8_t *ran_phase2, double *f0, double *maxviol, std::vector<int> &st, std::vector<int> &st1) {
    const int64_t R = c->R, bytes = 57 * R;
    int rco = cd_outputs_reserve(c, R);
    if (rco) return rco;
    hipLaunchKernelGGL(pack_cd_outputs_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, c->stream, c->d_out, R,
                       (const int64_t *)c->d_sweeps1, (const int64_t *)c->d_sweeps, (const int64_t *)c->d_visits,
                       (const int64_t *)c->d_acc, (const double *)c->d_f0, (const double *)c->d_mv,
                       (const int *)c->d_status, (const int *)c->d_status1, (const uint8_t *)c->d_flag);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_out, c->d_out, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    const char *h = c->h_out;
    const size_t n8 = (size_t)R * 8;
    if (sweeps1) memcpy(sweeps1, h, n8);
    if (sweeps2) memcpy(sweeps2, h + n8, n8);
    if (visits2) memcpy(visits2, h + 2 * n8, n8);
    if (accepted2) memcpy(accepted2, h + 3 * n8, n8);
    if (f0) memcpy(f0, h + 4 * n8, n8);
    if (maxviol) memcpy(maxviol, h + 5 * n8, n8);
    st.resize((size_t)R); st1.resize((size_t)R);
    memcpy(st.data(), h + 6 * n8, (size_t)R * 4);
    memcpy(st1.data(), h + 6 * n8 + (size_t)R * 4, (size_t)R * 4);
    if (ran_phase2) memcpy(ran_phase2, h + 7 * n8, (size_t)R);
    return 0;
}

// Per-restart status policy of a coordinate-descent run.  A restart on which the reference would raise
// (code != 0) is a FAILED restart, not a failed population: its objective / max violation become +inf (host
// outputs and the device copies select_best reads), the codes stay readable through qcqpmi_cd_status.  The call
// itself fails -- with the reference's message -- only when every restart failed (in particular R == 1, the
// reference's single-point behaviour).
int cd_apply_status(qcqpmi_ctx *c, const std::vector<int> &st, const std::vector<int> &st1, double *f0, double *maxviol,
                    int seg_cap) {
    const int64_t R = c->R;
    c->last_st1 = st1; c->last_st2 = st;
    int64_t nfail = 0, first = -1;
    for (int64_t r = 0; r < R; r++)
        if (st1[(size_t)r] || st[(size_t)r]) { if (first < 0) first = r; nfail++; }
    if (nfail == 0) return 0;
    if (nfail < R) {
        const double inf = INFINITY;
        for (int64_t r = 0; r < R; r++) {
            if (!(st1[(size_t)r] || st[(size_t)r])) continue;
            if (f0) f0[r] = inf;
            if (maxviol) maxviol[r] = inf;
            HIPCHK(c, hipMemcpyAsync(c->d_f0 + r, &inf, sizeof(double), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->d_mv + r, &inf, sizeof(double), hipMemcpyHostToDevice, c->stream));
        }
        HIPCHK(c, spin_sync(c->stream));
        return 0;
    }
    const int64_t r = first;
    const int s1 = st1[(size_t)r], s2 = st[(size_t)r];
    if (s1 == -3) return fail(c, QCQPMI_EREFERENCE, "phase 1: a variable appears in no constraint (reference: ValueError: max() arg is an empty sequence, qcqp.py:117); restart %lld", (long long)r);
    if (s1 == -4 || s2 == -4) return fail(c, QCQPMI_EUNSUPPORTED, "feasible set with more than %d segments; restart %lld", seg_cap, (long long)r);
    if (s1) return fail(c, QCQPMI_EREFERENCE, "phase 1: unbounded feasible interval with zero objective (reference: OverflowError in np.random.uniform, utilities.py:267); restart %lld", (long long)r);
    return fail(c, QCQPMI_EREFERENCE, "phase 2: the reference raises on restart %lld (code %d: unbounded interval with zero objective / NameError in OneVarQuadraticFunction.eval)", (long long)r, s2);
}

void cd_queue_fill_batch(qcqpmi_ctx *c, CdBatch &B, uint64_t seed, uint64_t first_index) {
    B.X = c->X; B.f0cur = c->d_f0; B.slack = c->d_mv; B.flag = c->d_flag; B.visits = c->d_visits; B.accepted = c->d_acc;
    B.sweeps = c->d_sweeps; B.status = c->d_status; B.f0out = c->d_f0; B.mvout = c->d_mv; B.R = c->R; B.seed = seed;
    B.first_index = first_index; B.next = c->d_qnext;
}

// does the round-4 slot-queue kernel take the problem's shape?  (the switches are the caller's: cd_queue_eligible for qcqpmi_cd_run,
// stream_plan for the lifecycle mode of qcqpmi_cd_stream_run)
bool cd_queue_shape_ok(const qcqpmi_ctx *c) {
    if (!c->sep || c->maxc > 1) return false;
    if (!(c->K == 1 && c->objclass == 1 && c->symcls && c->n % 16 == 0)) return false;
    return cd_queue_lds_bytes(c->dp) != 0 && c->R < (1LL << 30);
}

void launch_gate(qcqpmi_ctx *c, double viol_tol) {
    hipLaunchKernelGGL(gate_kernel, dim3((unsigned)((c->Rpad + 255) / 256)), dim3(256), 0, c->stream, c->d_mv,
                       c->d_status1, c->d_flag, c->R, c->Rpad, viol_tol);
}

}  // namespace qcqpmi

namespace {

// does phase 2 of the resident population go through the slot-queue kernel?
bool cd_queue_eligible(qcqpmi_ctx *c, bool profiling) {      // the problem's shape and the context's switches allow the kernel
    if (profiling || c->force_generic || (c->dbg & 64) || c->cd_queue == 0) return false;
    return cd_queue_shape_ok(c);
}

bool cd_queue_applies(qcqpmi_ctx *c, bool profiling) {
    if (!cd_queue_eligible(c, profiling)) return false;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess) return false;
    if (c->cd_queue == 1) return true;
    if (c->cd_queue == 2) return c->Rpad / 16 > cus;
    return false;
}

// reset the queue of the resident population and the per-restart outputs the kernel only writes for the restarts it runs,
// then publish the population (generation number) to whoever may pull from it
int cd_queue_prepare(qcqpmi_ctx *c) {
    HIPCHK(c, c->d_qnext.reserve(c->stream, 16));
    HIPCHK(c, hipMemsetAsync(c->d_visits, 0, (size_t)c->Rpad * sizeof(int64_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_acc, 0, (size_t)c->Rpad * sizeof(int64_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_sweeps, 0, (size_t)c->Rpad * sizeof(int64_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_status, 0, (size_t)c->Rpad * sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_qnext, 0, 16 * sizeof(int), c->stream));
    c->q_prepared = true;
    return 0;
}

template <int MAXC>
int launch_cd(qcqpmi_ctx *c, const CdArgs &a1, bool phase1, bool &used_lds, bool *used_rs = nullptr) {
    if (used_rs) *used_rs = false;
    if (!phase1) c->last_cd2_kernel = "cd_phase2_kernel";
    const bool cd_debug = getenv("QCQPMI_CD_DEBUG") != nullptr;     // tests: one line per launch with the template arguments chosen below
    dim3 grid((unsigned)(c->Rpad / 16)), block(256);
    if (phase1) {
        if (cd_debug) fprintf(stderr, "launch_cd: cd_phase1_sep_kernel MAXC %d\n", MAXC);
        tic(c, 1);
        hipLaunchKernelGGL(cd_phase1_sep_kernel<MAXC>, grid, dim3(P1_THREADS), 0, c->stream, a1);
        toc(c, 1);
        HIPCHK(c, hipGetLastError());
        return 0;
    }
    const DevProblem &dp = c->dp;
    // second-generation role-split kernel (cd_phase2_q.h): one mirrored equality class, positive diagonal, n a
    // multiple of 16, the tile resident in LDS -- the Boolean least squares family of the headline benchmark
    if (MAXC == 1 && c->K == 1 && c->objclass == 1 && c->symcls && c->n % 16 == 0 && !c->force_generic && !(c->dbg & 64)) {
        // (at least RQ_LDS_MIN: the product loop's look-ahead loads address a full-size tile)
        size_t q_lds = ((size_t)RQ_LDS_COMMON + (size_t)c->n16 * 16) * sizeof(double);
        if (q_lds < RQ_LDS_MIN) q_lds = RQ_LDS_MIN;
        const int NBq = (int)(c->n16 / 16);
        const int cs = chain_share(NBq, c->dbg);
        if (cd_queue_applies(c, a1.prof != nullptr) && chain_range_ok(NBq, cs)) {
            // restart-level scheduling (cd_queue.h): 16 slots per workgroup, refilled from a device-side queue
            used_lds = true;
            int rcq;
            if (!c->q_prepared && (rcq = cd_queue_prepare(c))) return rcq;
            c->q_prepared = false;
            CdQueueArgs qa;
            qa.P = dp; qa.num_iters = a1.num_iters; qa.tol = a1.tol; qa.life = nullptr; qa.life_on = 0;
            cd_queue_fill_batch(c, qa.b, a1.seed, a1.first_index);
            if (cd_debug) fprintf(stderr, "launch_cd: cd_phase2_qs_kernel CS %d\n", cs);
            int cus = 0;
            HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
            (void)hipEventRecord(c->timers[2].beg, c->stream);
            hipError_t qe = (hipError_t)cd_queue_launch(qa, cs, cus, c->stream);
            (void)hipEventRecord(c->timers[2].end, c->stream);
            c->timers[2].valid = true;
            if (qe != hipSuccess) return fail(c, QCQPMI_EHIP, "cd_queue_launch: %s", hipGetErrorString(qe));
            c->last_cd2_kernel = "cd_phase2_qs_kernel";
            if (used_rs) *used_rs = true;
            return 0;
        }
        if (q_lds <= 160 * 1024 && chain_range_ok(NBq, cs)) {
            used_lds = true;
            const bool prof_ = a1.prof != nullptr;
            auto k = cd_phase2_q_kernel<4, false>;
            if (prof_) k = cs == 0 ? cd_phase2_q_kernel<0, true> : cs == 2 ? cd_phase2_q_kernel<2, true> : cs == 4 ? cd_phase2_q_kernel<4, true> : cd_phase2_q_kernel<6, true>;
            else k = cs == 0 ? cd_phase2_q_kernel<0, false> : cs == 2 ? cd_phase2_q_kernel<2, false> : cs == 4 ? cd_phase2_q_kernel<4, false> : cd_phase2_q_kernel<6, false>;
            HIPCHK(c, hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)q_lds));
            if (cd_debug) fprintf(stderr, "launch_cd: cd_phase2_q_kernel CS %d\n", cs);
            tic(c, 2);
            hipLaunchKernelGGL(k, grid, dim3(512), q_lds, c->stream, a1, dp.Apack, dp.Apack2, dp.P0, dp.q0, dp.rcp2d);
            toc(c, 2);
            c->last_cd2_kernel = "cd_phase2_q_kernel";
            HIPCHK(c, hipGetLastError());
            if (used_rs) *used_rs = true;
            return 0;
        }
    }
    // role-split pipelined kernel for the single-class Boolean / box families
    if (MAXC == 1 && c->K == 1 && (c->objclass == 1 || c->objclass == 2) && !c->force_generic) {
        const size_t rs_common = (size_t)(2 * 6 * 256 + 256 + 2 * 256 + 2 * 16 + 2 * 16 + 16 + 4 * 16 + 8 + 8 + 8) * sizeof(double);
        const size_t rs_with_x = rs_common + (size_t)c->n16 * 16 * sizeof(double);
        used_lds = rs_with_x <= 160 * 1024;
        const size_t rs_lds = used_lds ? rs_with_x : rs_common;
        dim3 block512(512);
#define QM_RS(XL, FA)                                                                               \
    do {                                                                                            \
        auto k = cd_phase2_rs_kernel<XL, FA, false, false, false>;                                  \
        const bool full_ = (c->n % 16 == 0), sym_ = c->symcls, prof_ = a1.prof != nullptr;          \
        if (prof_) k = full_ ? (sym_ ? cd_phase2_rs_kernel<XL, FA, true, true, true> : cd_phase2_rs_kernel<XL, FA, true, false, true>) \
                             : (sym_ ? cd_phase2_rs_kernel<XL, FA, false, true, true> : cd_phase2_rs_kernel<XL, FA, false, false, true>); \
        else k = full_ ? (sym_ ? cd_phase2_rs_kernel<XL, FA, true, true, false> : cd_phase2_rs_kernel<XL, FA, true, false, false>) \
                       : (sym_ ? cd_phase2_rs_kernel<XL, FA, false, true, false> : cd_phase2_rs_kernel<XL, FA, false, false, false>); \
        HIPCHK(c, hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rs_lds)); \
        if (cd_debug) fprintf(stderr, "launch_cd: cd_phase2_rs_kernel XL %d FA %d FULL %d SYM %d\n", (int)XL, FA, (int)full_, (int)sym_); \
        tic(c, 2);                                                                                  \
        hipLaunchKernelGGL(k, grid, block512, rs_lds, c->stream, a1, dp.Apack, dp.Apack2, dp.P0, dp.q0, dp.rcp2d); \
        toc(c, 2);                                                                                  \
    } while (0)
        if (used_lds && c->objclass == 1) QM_RS(true, 1);
        else if (used_lds) QM_RS(true, 2);
        else if (c->objclass == 1) QM_RS(false, 1);
        else QM_RS(false, 2);
#undef QM_RS
        c->last_cd2_kernel = "cd_phase2_rs_kernel";
        HIPCHK(c, hipGetLastError());
        if (used_rs) *used_rs = true;
        return 0;
    }
    // dynamic LDS: [X tile] + partial tiles + G + diagonal block + slack + feasible-set table
    const bool use_cls = c->K <= 16;
    const size_t slots = use_cls ? (size_t)c->K * 16 : 0;
    size_t common = (size_t)(4 * 256 + 256 + 256 + 3 * 16 + 512) * sizeof(double) +              // part, G, Dblk, slk/q0b/rcpb, midb/thrb
                    (size_t)(2 * (MAXC + 1) * 256 + 256) * sizeof(double) +                      // block table
                    ((size_t)(2 * (MAXC + 1)) * slots + ((slots + 1) / 2) * 2) * sizeof(double) + // class table
                    64;
    size_t with_x = common + (size_t)c->n16 * 16 * sizeof(double);
    used_lds = with_x <= 160 * 1024;
    const size_t lds = used_lds ? with_x : common;
    const int fast = (MAXC == 1) ? c->objclass : 0;
    const bool uni = use_cls && c->K == 1;
#define QM_LAUNCH2(XL, CL, FA, UN)                                                                     \
    do {                                                                                            \
        auto k = cd_phase2_kernel<MAXC, XL, CL, FA, UN>;                                                \
        HIPCHK(c, hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        if (cd_debug) fprintf(stderr, "launch_cd: cd_phase2_kernel MAXC %d XL %d CL %d FA %d UN %d\n", MAXC, (int)XL, (int)CL, FA, (int)UN); \
        tic(c, 2);                                                                                  \
        hipLaunchKernelGGL(k, grid, block, lds, c->stream, a1, dp.Apack, dp.P0, dp.q0, dp.rcp2d, dp.cls);      \
        toc(c, 2);                                                                                  \
    } while (0)
#define QM_LAUNCH(XL, CL)                                                 \
    do {                                                                  \
        if (fast == 1 && uni && CL) QM_LAUNCH2(XL, CL, 1, CL);            \
        else if (fast == 2 && uni && CL) QM_LAUNCH2(XL, CL, 2, CL);       \
        else if (fast == 1) QM_LAUNCH2(XL, CL, 1, false);                 \
        else if (fast == 2) QM_LAUNCH2(XL, CL, 2, false);                 \
        else QM_LAUNCH2(XL, CL, 0, false);                                \
    } while (0)
    if (used_lds && use_cls) QM_LAUNCH(true, true);
    else if (used_lds) QM_LAUNCH(true, false);
    else if (use_cls) QM_LAUNCH(false, true);
    else QM_LAUNCH(false, false);
#undef QM_LAUNCH
#undef QM_LAUNCH2
    HIPCHK(c, hipGetLastError());
    return 0;
}

// coordinate descent for constraints that couple coordinates (cd_general.h)
int cd_run_general(qcqpmi_ctx *c, int phase1, int64_t num_iters, double viol_tol, double tol, uint64_t seed,
                   uint64_t first_index, int64_t *sweeps1, int64_t *sweeps2, int64_t *visits2, int64_t *accepted2,
                   uint8_t *ran_phase2, double *f0, double *maxviol) {
    if (!c->d_gP) return fail(c, QCQPMI_EUNSUPPORTED, "coupled constraints: dense storage m*n*n exceeds 16 GB");
    if (num_iters < 0 || !(tol > 0.0)) return fail(c, QCQPMI_EINVAL, "cd_run: bad num_iters / tol");
    const int64_t m = c->m;
    const size_t lds = ((size_t)(m + 1) * 16 * 4 + 4 * 16 * GEN_CAP + 16 * GEN_CAP + 16) * sizeof(double);
    if (lds > 160 * 1024) return fail(c, QCQPMI_EUNSUPPORTED, "coupled constraints: m = %lld too large for the LDS-resident coefficient table", (long long)m);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    CdGenArgs g;
    CdArgs &a = g.b;
    a.P = c->dp; a.X = c->X; a.R = c->R; a.f0cur = c->d_f0; a.slack = c->d_mv;
    a.num_iters = num_iters; a.viol_tol = viol_tol; a.tol = tol; a.seed = seed; a.first_index = first_index;
    a.visits = c->d_visits; a.accepted = c->d_acc; a.sweeps = c->d_sweeps; a.status = c->d_status;
    a.flag = c->d_flag; a.prof = nullptr; a.dbg = 0; a.f0out = nullptr; a.mvout = nullptr;
    g.gP = c->d_gP; g.Rpad = c->Rpad;
    g.exact_t0 = ((c->n <= 64 || c->cd_ref_order) && !(c->dbg & 16)) ? 1 : 0;   // small problems (or on request): the reference's own arithmetic for t0
    dim3 grid((unsigned)(c->Rpad / 16)), block(256);
    auto k1 = cd_general_kernel<1>;
    auto k2 = cd_general_kernel<2>;
    HIPCHK(c, hipFuncSetAttribute((const void *)k1, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(c, hipFuncSetAttribute((const void *)k2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(c, hipMemsetAsync(c->d_sweeps1, 0, (size_t)c->Rpad * sizeof(int64_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_status1, 0, (size_t)c->Rpad * sizeof(int), c->stream));
    if (phase1) {
        if ((rc = launch_eval(c, true))) return rc;
        g.F = c->d_F;
        CdGenArgs g1 = g;
        g1.b.sweeps = c->d_sweeps1;
        g1.b.status = c->d_status1;
        tic(c, 1);
        hipLaunchKernelGGL(k1, grid, block, lds, c->stream, g1);
        toc(c, 1);
        HIPCHK(c, hipGetLastError());
    }
    if ((rc = launch_eval(c, true))) return rc;
    g.F = c->d_F;
    launch_gate(c, viol_tol);
    HIPCHK(c, hipGetLastError());
    if (ran_phase2) HIPCHK(c, hipMemcpyAsync(ran_phase2, c->d_flag, (size_t)c->R, hipMemcpyDeviceToHost, c->stream));
    tic(c, 2);
    hipLaunchKernelGGL(k2, grid, block, lds, c->stream, g);
    toc(c, 2);
    HIPCHK(c, hipGetLastError());
    if ((rc = launch_eval(c, false))) return rc;
    std::vector<int> st, st1;
    if ((rc = fetch_cd_outputs(c, sweeps1, sweeps2, visits2, accepted2, nullptr, f0, maxviol, st, st1))) return rc;
    if ((rc = cd_apply_status(c, st, st1, f0, maxviol, GEN_CAP))) return rc;
    return 0;
}

}  // namespace

// ============================================================================================

extern "C" {

// ------------------------------------------------------------------------- coordinate descent

// stage 0: the whole run.  Stages 1-3 split it for callers that overlap the preparation of the NEXT population with the
// phase-2 kernel of the current one (two contexts = two streams): 1 = phase 1 + evaluation + gate (asynchronous),
// 2 = launch of phase 2 (asynchronous), 3 = results (blocking).  Paths without a pipelined phase-2 kernel run everything
// in stage 3.
int qcqpmi_cd_run_stage(qcqpmi_ctx *c, int stage, int phase1, int64_t num_iters, double viol_tol, double tol,
                        uint64_t seed, uint64_t first_index, int64_t *sweeps1, int64_t *sweeps2,
                        int64_t *visits2, int64_t *accepted2, uint8_t *ran_phase2, double *f0,
                        double *maxviol) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (stage < 0 || stage > 3) return fail(c, QCQPMI_EINVAL, "cd_run_stage: stage %d", stage);
    if (stage >= 2 && c->cd_stage != stage - 1) return fail(c, QCQPMI_ESTATE, "cd_run_stage: stage %d without stage %d", stage, stage - 1);
    const bool whole = dense_on(c) || !c->sep;      // these paths are not split
    if (whole) {
        if (stage == 1 || stage == 2) { c->cd_stage = stage; return 0; }
        c->cd_stage = 0;
        c->last_cd2_kernel = (dense_on(c) && !c->cd_ref_order) ? dense_chain_name(c) : "cd_general_kernel";
        if (c->cd_ref_order && !c->d_gP)
            return fail(c, QCQPMI_EUNSUPPORTED, "reference-order coordinate descent needs the row-major constraint matrices "
                        "(uploaded functions, m n^2 <= 2e9 entries); device-generated functions only exist packed");
        if (dense_on(c) && !c->cd_ref_order) return cd_run_dense(c, phase1, num_iters, viol_tol, tol, seed, first_index, sweeps1, sweeps2, visits2,
                                             accepted2, ran_phase2, f0, maxviol);
        return cd_run_general(c, phase1, num_iters, viol_tol, tol, seed, first_index, sweeps1, sweeps2, visits2,
                              accepted2, ran_phase2, f0, maxviol);
    }
    if (num_iters < 0 || !(tol > 0.0)) return fail(c, QCQPMI_EINVAL, "cd_run: bad num_iters / tol");
    HIPCHK(c, hipSetDevice(c->device));
    CdArgs a;
    a.P = c->dp; a.X = c->X; a.R = c->R; a.f0cur = c->d_f0; a.slack = c->d_mv;
    a.num_iters = num_iters; a.viol_tol = viol_tol; a.tol = tol; a.seed = seed; a.first_index = first_index;
    a.visits = c->d_visits; a.accepted = c->d_acc; a.sweeps = c->d_sweeps; a.status = c->d_status;
    a.flag = c->d_flag;
    a.prof = nullptr; a.f0out = nullptr; a.mvout = nullptr;
    a.dbg = c->dbg;
    bool used_lds = false;
    // Everything below is enqueued on the context's stream without a host round trip: phase 1,
    // evaluation, the improve_coord_descent gate, phase 2, final evaluation, result copies.
    if (stage == 0 || stage == 1) {
        HIPCHK(c, hipMemsetAsync(c->d_sweeps1, 0, (size_t)c->Rpad * sizeof(int64_t), c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_status1, 0, (size_t)c->Rpad * sizeof(int), c->stream));
        if (phase1) {
            CdArgs a1 = a;
            a1.sweeps = c->d_sweeps1;
            a1.status = c->d_status1;
            rc = (c->maxc <= 1) ? launch_cd<1>(c, a1, true, used_lds) : launch_cd<4>(c, a1, true, used_lds);
            if (rc) return rc;
        }
        // gate of improve_coord_descent (qcqp.py:189): phase 2 only if max violation < viol_tol.
        // The evaluation also provides the phase-2 slack (qcqp.py:157) and the running objective.
        if ((rc = launch_eval(c, false))) return rc;
        launch_gate(c, viol_tol);
        HIPCHK(c, hipGetLastError());
        c->q_prepared = false;
        if (cd_queue_applies(c, c->profile) && (rc = cd_queue_prepare(c))) return rc;     // queue reset + population published
        if (stage == 1) { c->cd_stage = 1; return 0; }
    }
    if (stage == 0 || stage == 2) {
        if (c->profile) {
            const size_t words = (size_t)(c->Rpad / 16) * 16 + QCQPMI_TRACE_WORDS;
            HIPCHK(c, c->d_prof.reserve(c->stream, words, false));
            HIPCHK(c, hipMemsetAsync(c->d_prof, 0, words * sizeof(long long), c->stream));
            a.prof = c->d_prof;
        }
        // the pipelined kernel leaves objective and max violation of the restarts it ran in place (tracked objective,
        // element-wise violations of the final tile): no evaluation pass afterwards
        bool used_rs = false;
        a.f0out = c->d_f0; a.mvout = c->d_mv;
        rc = (c->maxc <= 1) ? launch_cd<1>(c, a, false, used_lds, &used_rs) : launch_cd<4>(c, a, false, used_lds, &used_rs);
        if (rc) return rc;
        if (!used_rs && (rc = launch_eval(c, false))) return rc;
        if (stage == 2) { c->cd_stage = 2; return 0; }
    }
    c->cd_stage = 0;
    std::vector<int> st, st1;
    if ((rc = fetch_cd_outputs(c, sweeps1, sweeps2, visits2, accepted2, ran_phase2, f0, maxviol, st, st1))) return rc;
    if ((rc = cd_apply_status(c, st, st1, f0, maxviol, 0))) return rc;
    return 0;
}

int qcqpmi_cd_run(qcqpmi_ctx *c, int phase1, int64_t num_iters, double viol_tol, double tol,
                  uint64_t seed, uint64_t first_index, int64_t *sweeps1, int64_t *sweeps2,
                  int64_t *visits2, int64_t *accepted2, uint8_t *ran_phase2, double *f0,
                  double *maxviol) {
    return qcqpmi_cd_run_stage(c, 0, phase1, num_iters, viol_tol, tol, seed, first_index, sweeps1, sweeps2, visits2, accepted2,
                               ran_phase2, f0, maxviol);
}

int qcqpmi_cd_status(qcqpmi_ctx *c, int *status1, int *status2) {
    if (!c) return QCQPMI_EINVAL;
    if ((int64_t)c->last_st1.size() != c->R || (int64_t)c->last_st2.size() != c->R)
        return fail(c, QCQPMI_ESTATE, "cd_status: no coordinate-descent run on the resident population");
    if (status1) memcpy(status1, c->last_st1.data(), (size_t)c->R * sizeof(int));
    if (status2) memcpy(status2, c->last_st2.data(), (size_t)c->R * sizeof(int));
    return 0;
}

int qcqpmi_cd_queue(qcqpmi_ctx *c, int mode) {
    if (!c || mode < 0 || mode > 2) return QCQPMI_EINVAL;
    c->cd_queue = mode;
    return 0;
}

int qcqpmi_cd_reference_order(qcqpmi_ctx *c, int enable) {
    if (!c) return QCQPMI_EINVAL;
    c->cd_ref_order = enable != 0;
    return 0;
}

int qcqpmi_debug_profile(qcqpmi_ctx *c, int enable, int64_t *sums8) {
    if (!c) return QCQPMI_EINVAL;
    c->profile = (enable & 1) != 0;
    c->force_generic = (enable & 2) != 0;
    c->dbg = enable >> 4;
    if (sums8 && c->d_prof && c->Rpad > 0) {
        std::vector<long long> h((size_t)(c->Rpad / 16) * 16);
        HIPCHK(c, hipMemcpy(h.data(), c->d_prof, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
        for (int k = 0; k < 16; k++) sums8[k] = 0;
        for (size_t t = 0; t < h.size(); t++) sums8[t & 15] += h[t];
    }
    return 0;
}

// debug: event trace of tile 0 written by the profiled phase-2 kernel (8 slices of 256 words, one per wave: entries of
// 4 timestamps per block / product; see cd_phase2_q.h)
int qcqpmi_debug_trace(qcqpmi_ctx *c, int64_t *out, int count) {
    if (!c || !out || count < 0 || count > QCQPMI_TRACE_WORDS) return QCQPMI_EINVAL;
    if (!c->d_prof || c->Rpad <= 0) return fail(c, QCQPMI_EINVAL, "no profiled run to trace");
    HIPCHK(c, hipMemcpy(out, c->d_prof + (size_t)(c->Rpad / 16) * 16, (size_t)count * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
