// Streamed coordinate descent of the C ABI: K populations of R restarts through ONE persistent slot-queue launch (cd_queue.h, CdLife) --
// qcqpmi_cd_stream_run, qcqpmi_cd_stream_reserve and the switches that only they read (the objective factor, the kernel version, the
// tick sums).  Host code only: the kernels are launched by the units that compile them (cd_life.hip, cd_queue.hip; select_best_kernel and
// gather_best_x_kernel through the launchers of capi.hip).  What a run launches and needs is decided in ONE place, stream_plan
// (cd_life_plan.h: plain C++, tested on the CPU); reserve and run both consume that plan.
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "capi_ctx.h"
#include "cd_life.h"      // the launchers of cd_life.hip; with it cd_life_plan.h and the launcher of cd_queue.hip (cd_queue.h)

using namespace qcqpmi;

namespace {

StreamShape stream_shape(const qcqpmi_ctx *c) {
    StreamShape s;
    s.NB = (int)(c->n16 / 16); s.sep = c->sep; s.maxc = c->maxc; s.Kreal = c->Kreal; s.objclass = c->objclass; s.symcls = c->symcls;
    s.queue_ok = cd_queue_shape_ok(c);
    return s;
}

// the ONE place where the streamed path reads the environment (QCQPMI_L2_CS and QCQPMI_L2_DEBUG are the launcher's own: cd_life2_launch)
StreamSwitches stream_switches(const qcqpmi_ctx *c) {
    StreamSwitches s;
    s.life_version = c->life_version; s.force_generic = c->force_generic; s.dbg = c->dbg; s.lr_RB = c->lr_RB; s.profile = c->profile;
    const char *ev = getenv("QCQPMI_L2_PREBUILT");
    s.prebuilt = !(ev && atoi(ev) == 0);
    ev = getenv("QCQPMI_L2_Y0_MAX");
    s.y0_max = ev ? atoll(ev) : STREAM_Y0_ALL;
    ev = getenv("QCQPMI_L2_ROT");
    s.rot = ev ? atoi(ev) : STREAM_ROT_AUTO;
    ev = getenv("QCQPMI_L2_TILES");
    s.tiles = ev ? atoi(ev) : 0;
    return s;
}

int stream_plan_for(qcqpmi_ctx *c, int64_t K, int64_t R, StreamPlan *P) {
    int cus = 0;
    HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    *P = stream_plan(stream_shape(c), stream_switches(c), K, R, cus);
    return 0;
}

// device buffers of the per-population winners of a streamed run (K populations)
int cd_bestK_reserve(qcqpmi_ctx *c, size_t K) {
    HIPCHK(c, c->d_bestK_idx.reserve(c->stream, K * 2, false));
    HIPCHK(c, c->d_bestK_key.reserve(c->stream, K * 2, false));
    HIPCHK(c, c->d_bestK_x.reserve(c->stream, K * (size_t)c->n, false));
    return 0;
}

// buffers of cd_life_kernel: the workgroups' X tiles, the staged diagonal blocks (packed once per problem), the watchdog word
int cd_life2_reserve(qcqpmi_ctx *c, size_t scratch) {
    HIPCHK(c, c->l2_scratch.reserve(c->stream, scratch));
    HIPCHK(c, c->l2_abort.reserve(c->stream, 4));
    HIPCHK(c, c->l2_cuslot.reserve(c->stream, 4096));
    if (!c->l2_S) {      // (the second of the pair: a call that failed between the two starts over)
        const size_t NB = (size_t)(c->n16 / 16);
        HIPCHK(c, c->l2_D.reserve(c->stream, NB * 256));
        HIPCHK(c, c->l2_S.reserve(c->stream, NB * 48));
        hipError_t e = (hipError_t)cd_life2_pack(c->dp, c->l2_D, c->l2_S, c->stream);
        if (e != hipSuccess) return fail(c, QCQPMI_EHIP, "cd_life2_pack: %s", hipGetErrorString(e));
    }
    return 0;
}

// buffers of the pre-passes of a prebuilt factored run: the slacks (cd_life_prep_kernel) and Y0 (cd_life_y0_kernel)
int cd_life2_pre_reserve(qcqpmi_ctx *c, const StreamPlan &P) {
    HIPCHK(c, c->l2_preslack.reserve(c->stream, P.l2_preslack));
    HIPCHK(c, c->l2_y0.reserve(c->stream, P.l2_y0, false));      // (every element a restart reads is written by the pre-pass)
    return 0;
}

// every buffer the planned run needs beyond the resident population (the tick sums of a profiled run apart: they are zeroed where they
// are handed to the launch); winners: the per-population winners too.  qcqpmi_cd_stream_reserve does this for a caller that wants no
// allocation in the run.
int stream_reserve(qcqpmi_ctx *c, const StreamPlan &P, bool winners) {
    int rc;
    if (P.outputs && (rc = cd_outputs_reserve(c, (int64_t)P.outputs))) return rc;
    if (winners && P.bestK && (rc = cd_bestK_reserve(c, P.bestK))) return rc;
    HIPCHK(c, c->d_qnext.reserve(c->stream, 16));
    HIPCHK(c, c->d_life.reserve(c->stream, 1, false));
    if (P.kernel == STREAM_LIFE2 && (rc = cd_life2_reserve(c, P.l2_scratch))) return rc;
    if (P.pre && (rc = cd_life2_pre_reserve(c, P))) return rc;
    return 0;
}

// QCQPMI_STREAM_TIMING=1: host-side wall clock of the call's stages on stderr (set-up, kernel, fetch, status, best), and of the steps of
// the lifecycle launch
struct StreamClock {
    const bool on = getenv("QCQPMI_STREAM_TIMING") != nullptr;
    double stage[6] = {0, 0, 0, 0, 0, 0}, step[6] = {0, 0, 0, 0, 0, 0};
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void at_stage(int k) { stage[k] = now(); }
    void at_step(int k) { step[k] = now(); }
    void report_launch() const {      // after at_step(0..5); the steps follow stage 1
        if (on) fprintf(stderr, "cd_stream_run launch (ms): reserve %.3f, event %.3f, launch call %.3f, event + spin wait %.3f, copy call %.3f, sync %.3f\n", step[0] - stage[1], step[1] - step[0], step[2] - step[1], step[3] - step[2], step[4] - step[3], step[5] - step[4]);
    }
    void report() const {
        if (on) fprintf(stderr, "cd_stream_run timing (ms): set-up %.3f, launch + kernel %.3f, fetch %.3f, status %.3f, best %.3f\n", stage[1] - stage[0], stage[2] - stage[1],
                        stage[3] - stage[2], stage[4] - stage[3], stage[5] - stage[4]);
    }
};

struct StreamRun {               // the arguments of a run that the launch reads
    int64_t K, R, num_iters;
    double tol;
    uint64_t seed, first_index;
};

// the parameters of the lifecycle launch -> c->d_life
int stream_fill_life(qcqpmi_ctx *c, const StreamPlan &P, const StreamRun &r, int generate, int phase1, double viol_tol, uint64_t seed_stride,
                     uint64_t first_stride) {
    HIPCHK(c, hipMemsetAsync(c->d_qnext, 0, 16 * sizeof(int), c->stream));
    CdLife L;
    L.on = 1; L.generate = generate ? 1 : 0; L.phase1 = phase1 ? 1 : 0; L.Rtotal = r.K * r.R; L.Rpop = r.R;
    L.seed = r.seed; L.seed_stride = seed_stride; L.first_index = r.first_index; L.first_stride = first_stride; L.viol_tol = viol_tol;
    L.sweeps1 = c->d_sweeps1; L.status1 = c->d_status1; L.ran2 = c->d_flag;
    L.prof = nullptr;
    L.prebuilt = P.pre ? 1 : 0; L.preslack = P.pre ? (const double *)c->l2_preslack : nullptr;
    L.y0_count = P.y0_count; L.y0 = P.pre ? (const double *)c->l2_y0 : nullptr;
    if (P.life_prof) {      // qcqpmi_debug_profile: tick sums of the launch (qcqpmi_debug_life_profile)
        HIPCHK(c, c->d_life_prof.reserve(c->stream, P.life_prof, false));
        HIPCHK(c, hipMemsetAsync(c->d_life_prof, 0, P.life_prof * sizeof(long long), c->stream));
        L.prof = c->d_life_prof;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_life, &L, sizeof(L), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, spin_sync(c->stream));       // (L lives on this stack frame)
    return 0;
}

// cd_life_kernel behind its pre-passes, and the watchdog word afterwards
int stream_launch_life2(qcqpmi_ctx *c, const StreamPlan &P, const StreamRun &r, StreamClock &clk) {
    CdLife2Args qa;
    qa.P = c->dp; qa.num_iters = r.num_iters; qa.tol = r.tol; qa.life = c->d_life;
    cd_queue_fill_batch(c, qa.b, r.seed, r.first_index);
    qa.b.R = r.K * r.R;
    qa.scratch = c->l2_scratch; qa.Dpack = c->l2_D; qa.Spack = c->l2_S; qa.abort = c->l2_abort; qa.fbound = c->fbound;
    qa.cuslot = P.rot ? (int *)c->l2_cuslot : nullptr; qa.rotmode = P.rot;      // (stream_plan: what the second workgroup of a CU does)
    if (qa.cuslot) HIPCHK(c, hipMemsetAsync(c->l2_cuslot, 0, 4096 * sizeof(int), c->stream));
    qa.dbg = (c->dbg & 2048) ? 1 : 0;
    qa.Gpack = P.lr ? (const double *)c->lr_G : nullptr; qa.Upack = P.lr ? (const double *)c->lr_U : nullptr; qa.RB = P.lr ? c->lr_RB : 0;
    qa.nclass = c->Kreal;
    clk.at_step(0);
    (void)hipEventRecord(c->timers[2].beg, c->stream);       // (the event window spans the pre-pass too)
    clk.at_step(1);
    hipError_t qe = P.pre ? (hipError_t)cd_life2_prep_launch(c->dp, c->d_life, c->X, r.K * r.R, r.num_iters, r.tol, c->stream) : hipSuccess;
    if (qe == hipSuccess && P.y0_count > 0)
        qe = (hipError_t)cd_life2_y0_launch(c->X, c->lr_U, c->l2_y0, (int)(c->n16 / 16), P.factor_rb, c->n16, P.y0_count, c->stream);
    if (qe == hipSuccess) qe = (hipError_t)cd_life2_launch(qa, P.nmw, P.cs, P.kind, P.tiles, (int)P.wgs, c->stream);
    clk.at_step(2);
    (void)hipEventRecord(c->timers[2].end, c->stream);
    c->timers[2].valid = true;
    if (qe != hipSuccess) return fail(c, QCQPMI_EHIP, "cd_stream_run: %s", hipGetErrorString(qe));
    c->last_cd2_kernel = P.name;
    int ab = 0;
    HIPCHK(c, spin_sync(c->stream));
    clk.at_step(3);
    HIPCHK(c, hipMemcpyAsync(&ab, c->l2_abort, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    clk.at_step(4);
    HIPCHK(c, spin_sync(c->stream));
    clk.at_step(5);
    clk.report_launch();
    if (ab) {
        HIPCHK(c, hipMemsetAsync(c->l2_abort, 0, sizeof(int), c->stream));
        c->R = 0;
        return fail(c, QCQPMI_EHIP, "cd_stream_run: a wait inside cd_life_kernel ran into its watchdog (internal error; no results)");
    }
    return 0;
}

// cd_phase2_qs_kernel<CS, lifecycle>: the round-4 kernel (qcqpmi_cd_life_version(1))
int stream_launch_round4(qcqpmi_ctx *c, const StreamPlan &P, const StreamRun &r) {
    CdQueueArgs qa;
    qa.P = c->dp; qa.num_iters = r.num_iters; qa.tol = r.tol;
    qa.life = c->d_life; qa.life_on = 1;
    cd_queue_fill_batch(c, qa.b, r.seed, r.first_index);
    qa.b.R = r.K * r.R;
    (void)hipEventRecord(c->timers[2].beg, c->stream);
    hipError_t qe = (hipError_t)cd_queue_launch(qa, P.cs, (int)P.wgs, c->stream);
    (void)hipEventRecord(c->timers[2].end, c->stream);
    c->timers[2].valid = true;
    if (qe != hipSuccess) return fail(c, QCQPMI_EHIP, "cd_stream_run: %s", hipGetErrorString(qe));
    HIPCHK(c, spin_sync(c->stream));
    c->last_cd2_kernel = P.name;
    return 0;
}

// the best restart of every population (QCQPForm.better folded over it, ties -> lowest index): one workgroup per population, then one
// gather of the winners' columns -- three launches and three copies whatever K
int stream_select_best(qcqpmi_ctx *c, int64_t K, int64_t R, double select_tol, int64_t *best_index, double *best_f0, double *best_maxviol,
                       double *best_x) {
    launch_select_best(c, K, c->d_f0, c->d_mv, R, select_tol, c->d_bestK_idx, c->d_bestK_key);
    if (best_x) {
        HIPCHK(c, hipMemsetAsync(c->d_bestK_x, 0, (size_t)K * c->n * sizeof(double), c->stream));
        launch_gather_best_x(c, K, R, (const int64_t *)c->d_bestK_idx, c->d_bestK_x);
    }
    HIPCHK(c, hipGetLastError());
    std::vector<int64_t> idx((size_t)K * 2);
    std::vector<double> key((size_t)K * 2);
    HIPCHK(c, hipMemcpyAsync(idx.data(), c->d_bestK_idx, idx.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(key.data(), c->d_bestK_key, key.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (best_x) HIPCHK(c, hipMemcpyAsync(best_x, c->d_bestK_x, (size_t)K * c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    for (int64_t p = 0; p < K; p++) {
        if (best_index) best_index[p] = idx[(size_t)2 * p];            // index WITHIN the population
        if (best_f0) best_f0[p] = key[(size_t)2 * p];
        if (best_maxviol) best_maxviol[p] = key[(size_t)2 * p + 1];
    }
    return 0;
}

}  // namespace

extern "C" {

// ---- lifecycle run: K populations of R restarts through ONE persistent slot-queue launch (cd_queue.h, CdLife)
// Takes (stream_plan, cd_life_plan.h): separable constraints, up to four classes with up to two constraints per coordinate on a diagonal
// of P0 that is positive everywhere or zero everywhere; ONE class with one constraint per coordinate on a diagonal of mixed sign (round 7,
// the SGN kind: no objective factor); 33 <= n <= 2304 (<= 4096 with a factor).  Anything else: QCQPMI_EUNSUPPORTED, nothing touched.
int qcqpmi_cd_stream_run(qcqpmi_ctx *c, int64_t K, int64_t R, int generate, int phase1, int64_t num_iters, double viol_tol, double tol,
                         uint64_t seed, uint64_t seed_stride, uint64_t first_index, uint64_t first_stride, double select_tol,
                         int64_t *sweeps1, int64_t *sweeps2, int64_t *visits2, int64_t *accepted2, uint8_t *ran_phase2, double *f0,
                         double *maxviol, int64_t *best_index, double *best_f0, double *best_maxviol, double *best_x) {
    int rc = check_ready(c, generate ? false : true);
    if (rc) return rc;
    if (K < 1 || R < 1 || num_iters < 0 || !(tol > 0.0) || K * R >= (1LL << 30)) return fail(c, QCQPMI_EINVAL, "cd_stream_run: bad K / R / num_iters / tol");
    if (!generate && c->R != K * R) return fail(c, QCQPMI_EINVAL, "cd_stream_run: the resident population has %lld points, K R = %lld", (long long)c->R, (long long)(K * R));
    HIPCHK(c, hipSetDevice(c->device));
    StreamClock clk;
    clk.at_stage(0);
    // ---- which kernel (decided BEFORE the resident population is touched: a refused call leaves the context as it was)
    StreamPlan P;
    if ((rc = stream_plan_for(c, K, R, &P))) return rc;
    if (!P.supported) {
        if (P.range_only) return fail(c, QCQPMI_EUNSUPPORTED, "cd_stream_run: n = %lld outside the range of cd_phase2_qs_kernel (n <= 1024, at least 3 blocks of 16)", (long long)c->n);
        return fail(c, QCQPMI_EUNSUPPORTED, "cd_stream_run: the lifecycle kernel needs separable constraints -- at most four classes of coordinates, at most two constraints "
                    "per coordinate --, a diagonal of P0 that is positive everywhere or zero everywhere (a diagonal of mixed sign: ONE class with one constraint "
                    "per coordinate only; with several classes or two constraints per coordinate it runs the serial path), and 33 <= n <= 2304: use qcqpmi_cd_run "
                    "per population");
    }
    const bool winners = best_index || best_f0 || best_maxviol || best_x;
    if (generate && (rc = pop_reserve(c, K * R))) return rc;
    if ((rc = stream_reserve(c, P, winners))) return rc;
    const StreamRun run = {K, R, num_iters, tol, seed, first_index};
    if ((rc = stream_fill_life(c, P, run, generate, phase1, viol_tol, seed_stride, first_stride))) return rc;
    clk.at_stage(1);
    if ((rc = P.kernel == STREAM_LIFE2 ? stream_launch_life2(c, P, run, clk) : stream_launch_round4(c, P, run))) return rc;
    c->cd_stage = 0;
    c->evaluated = true;                   // d_f0 / d_mv hold the values of the final points
    if (clk.on) { (void)spin_sync(c->stream); clk.at_stage(2); }
    std::vector<int> st, st1;
    if ((rc = fetch_cd_outputs(c, sweeps1, sweeps2, visits2, accepted2, ran_phase2, f0, maxviol, st, st1))) return rc;
    clk.at_stage(3);
    if ((rc = cd_apply_status(c, st, st1, f0, maxviol, 0))) return rc;
    clk.at_stage(4);
    if (winners && (rc = stream_select_best(c, K, R, select_tol, best_index, best_f0, best_maxviol, best_x))) return rc;
    clk.at_stage(5);
    clk.report();
    return 0;
}

// every buffer qcqpmi_cd_stream_run(K, R) will need, so that the run allocates nothing (a timed region does not begin with an allocation)
int qcqpmi_cd_stream_reserve(qcqpmi_ctx *c, int64_t K, int64_t R) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (K < 1 || R < 1 || K * R >= (1LL << 30)) return fail(c, QCQPMI_EINVAL, "cd_stream_reserve: bad K / R");
    HIPCHK(c, hipSetDevice(c->device));
    StreamPlan P;
    if ((rc = stream_plan_for(c, K, R, &P))) return rc;
    if (K * R > c->Rcap) { if ((rc = pop_reserve(c, K * R))) return rc; }       // (a resident population of that size or more stays)
    if (!P.supported) { P = StreamPlan(); P.outputs = (size_t)(K * R); P.bestK = (size_t)K; }      // a shape the run refuses: the population, the outputs and the winners all the same
    return stream_reserve(c, P, true);
}

int qcqpmi_debug_life_profile(qcqpmi_ctx *c, int64_t *out16) {
    if (!c || !out16) return QCQPMI_EINVAL;
    for (int k = 0; k < 24; k++) out16[k] = 0;
    if (!c->d_life_prof) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, spin_sync(c->stream));
    HIPCHK(c, hipMemcpy(out16, c->d_life_prof, 24 * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
}

int qcqpmi_cd_set_objective_factor(qcqpmi_ctx *c, const double *L, int64_t r) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, spin_sync(c->stream));
    c->lr_L.release(); c->lr_G.release(); c->lr_U.release();
    c->lr_RB = 0;
    if (!L || r == 0) return 0;                       // cleared
    if (r < 1 || r > c->n) return fail(c, QCQPMI_EINVAL, "cd_set_objective_factor: r = %lld outside 1 .. n", (long long)r);
    if (!cd_life2_factor_ok((int)(c->n16 / 16), r))
        return fail(c, QCQPMI_EUNSUPPORTED, "cd_set_objective_factor: the factored lifecycle kernel takes factors of at most 288 columns and n >= 128");
    const int64_t n = c->n, n16 = c->n16, r16 = (r + 15) / 16 * 16;
    const int RB = (int)(r16 / 16), NB = (int)(n16 / 16);
    HIPCHK(c, c->lr_L.reserve(c->stream, (size_t)n16 * r16));      // (zero-filled)
    HIPCHK(c, c->lr_G.reserve(c->stream, (size_t)NB * RB * 256, false));
    HIPCHK(c, c->lr_U.reserve(c->stream, (size_t)NB * RB * 256, false));
    HIPCHK(c, hipMemcpy2DAsync(c->lr_L, (size_t)r16 * sizeof(double), L, (size_t)r * sizeof(double), (size_t)r * sizeof(double), (size_t)n,
                               hipMemcpyHostToDevice, c->stream));
    hipError_t e = (hipError_t)cd_life2_pack_factor(c->lr_L, c->lr_G, c->lr_U, NB, RB, c->stream);
    if (e != hipSuccess) return fail(c, QCQPMI_EHIP, "cd_life2_pack_factor: %s", hipGetErrorString(e));
    HIPCHK(c, spin_sync(c->stream));      // (the 2-D copy may still be reading the caller's pages)
    c->lr_RB = RB;
    return 0;
}

int qcqpmi_cd_life_version(qcqpmi_ctx *c, int version) {
    if (!c || version < 0 || version > 3) return QCQPMI_EINVAL;      // (3: cd_life_kernel without the objective factor)
    c->life_version = version;
    return 0;
}

}  // extern "C"
