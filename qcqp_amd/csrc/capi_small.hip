// Small-problem batch part of the C ABI: B small problems over the context's constraint structure in ONE
// persistent launch of cd_small.hip, admm_small.hip, chain_small.hip, sdr_small.hip or spectral_small.hip (narrow and wide kernel; the ADMM setup kernels live there too).  A call works in a device buffer of its own
// (sb_work for CD and ADMM, ss_work for SDR, SPECTRAL and the ADMM setup): the resident population, its evaluation, its status codes and an installed ADMM basis are not touched,
// whether the call succeeds or is refused.
// A driver is: its argument checks, in their order, with their texts; ONE declaration of every array of the call on a BatchCall
// (batch_call.h: the layout of the work buffer, the copies, the ticket, the per-restart records and the ticket arithmetic, all run on
// the CPU by tests/host/batch_call_selftest.cpp); the scalars of its argument struct; its launch through the unit that owns the
// kernel (launchers: small_batch.h).  What the drivers share comes first.
// Host code only: the launcher headers, and the launch of the core's selection kernel through capi_ctx.h.
#include <cmath>
#include <cstring>

#include "capi_ctx.h"
#include "batch_call.h"
#include "cd_small.h"
#include "admm_small.h"
#include "chain_small.h"
#include "sdr_small.h"
#include "spectral_small.h"
#include "spectral_wide.h"
#include "admm_setup.h"

using namespace qcqpmi;

namespace {

int check_batch_context(qcqpmi_ctx *c, const char *name) {
    const int rc = check_ready(c, false);
    if (rc) return rc;
    if (!c->sep) return fail(c, QCQPMI_EUNSUPPORTED, "%s: the constraints are not separable (a constraint couples coordinates, or a coordinate carries more than 4)", name);
    return 0;
}

int check_batch_count(qcqpmi_ctx *c, const char *name, int64_t B, int64_t R) {
    if (B >= (1LL << 30) || R >= (1LL << 30) || B * R >= (1LL << 30)) return fail(c, QCQPMI_EINVAL, "%s: B R = %lld restarts, at most 2^30 - 1 per call", name, (long long)(B * R));
    return 0;
}

// cons [B][m][3] = (p, q, r) of constraint k of problem b: finite, and every constraint touches its coordinate
int check_batch_cons(qcqpmi_ctx *c, const char *name, const double *cons, int64_t B, int64_t m) {
    for (int64_t k = 0; k < B * m; k++) {
        const double p = cons[3 * k], q = cons[3 * k + 1], r = cons[3 * k + 2];
        if (!std::isfinite(p) || !std::isfinite(q) || !std::isfinite(r))
            return fail(c, QCQPMI_EINVAL, "%s: constraint %lld of problem %lld holds a coefficient that is not finite", name, (long long)(k % m + 1), (long long)(k / m));
        if (p == 0.0 && q == 0.0)
            return fail(c, QCQPMI_EINVAL, "%s: constraint %lld of problem %lld has p == 0 and q == 0: it touches no coordinate", name, (long long)(k % m + 1), (long long)(k / m));
    }
    return 0;
}

int check_batch_rhos(qcqpmi_ctx *c, const char *name, const double *rhos, int64_t B) {
    for (int64_t b = 0; b < B; b++)
        if (!(rhos[b] > 0.0) || !std::isfinite(rhos[b])) return fail(c, QCQPMI_EINVAL, "%s: rho of problem %lld is not positive and finite", name, (long long)b);
    return 0;
}

// the objectives of the B problems at the head of the work buffer: P0_b, q0_b, r0_b -- and behind P0_b the second matrix of the ADMM
// paths, Minv_b (Mslot set; Minvs == nullptr: no ADMM stage, no room)
template <class Args>
void declare_objectives(BatchCall &f, Args &a, int64_t B, int64_t n, const double *P0s, const double *q0s, const double *r0s,
                        const double *Minvs = nullptr, const double **Mslot = nullptr) {
    f.in(P0s, (size_t)B * n * n * 8, &a.P0s);
    if (Mslot) f.in(Minvs, (size_t)B * n * n * 8, Mslot);
    f.in(q0s, (size_t)B * n * 8, &a.q0s);
    f.in(r0s, (size_t)B * 8, &a.r0s);
}

// cap < 1 from a *_workgroups: -hipError_t
int occupancy_failed(qcqpmi_ctx *c, const char *name, int cap) {
    return fail(c, QCQPMI_EHIP, "%s: occupancy query failed: %s", name, hipGetErrorString((hipError_t)(-cap)));
}

int launch_failed(qcqpmi_ctx *c, const char *name, hipError_t e) { return fail(c, QCQPMI_EHIP, "%s: %s", name, hipGetErrorString(e)); }

// waits for the launch that has just been enqueued and fails if its ticket[1] is set: a matrix was not symmetric (with_minv: the
// kernel scans Minv_b too)
int check_symmetric(qcqpmi_ctx *c, const char *name, const int *ticket, bool with_minv) {
    int flags[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(flags, ticket, sizeof(flags), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return flags[1] ? fail(c, QCQPMI_EINVAL, "%s: %s is not symmetric (or holds a NaN)", name, with_minv ? "a matrix P0_b or Minv_b" : "an objective matrix P0_b") : 0;
}

// The best restart of every problem (QCQPForm.better folded over its R restarts, ties -> lowest index): where the caller wants its
// pieces (any pointer may be null; none: nothing runs), and where they lie in the work buffer
struct BatchBest {
    int64_t *index;
    double *f0, *maxviol, *x;
    int64_t *didx = nullptr;                 // [B][2] as select_best_kernel leaves it
    double *dkey = nullptr, *dx = nullptr;   // [B][2], [B][n]
    bool wanted() const { return index || f0 || maxviol || x; }
    void declare(BatchCall &f, int64_t B, int64_t n) {
        f.room((size_t)B * 2 * sizeof(int64_t), &didx);
        f.room((size_t)B * 2 * sizeof(double), &dkey);
        f.room((size_t)B * n * 8, &dx);
    }
};

// what the three restart calls declare behind their objectives -- the starts, the points, the record block, the ticket, the winners,
// the per-problem coefficients -- and the scalars their argument structs share
template <class Args>
void declare_restarts(qcqpmi_ctx *c, BatchCall &f, Args &a, BatchBest &best, char **records, size_t record_bytes, int64_t B, int64_t R, int generate,
                      const double *X0, double *X, const double *cons, uint64_t seed, uint64_t seed_stride, uint64_t first_index) {
    f.in(generate ? nullptr : X0, (size_t)B * R * c->n * 8, &a.X0);
    f.out(X, (size_t)B * R * c->n * 8, &a.X);
    f.room(record_bytes, records);
    f.ticket(&a.ticket);
    best.declare(f, B, c->n);
    f.in(cons, (size_t)B * c->m * 24, &a.cons);
    a.P = c->dp; a.B = B; a.R = R; a.generate = generate ? 1 : 0;
    a.seed = seed; a.seed_stride = seed_stride; a.first_index = first_index;
}

// enqueue: one workgroup per problem selects, then one gather of the winners' points
int select_batch_best(qcqpmi_ctx *c, const char *name, const BatchBest &b, const double *f0, const double *maxviol, const double *X,
                      int64_t B, int64_t R, int64_t n, double select_tol) {
    if (!b.wanted()) return 0;
    launch_select_best(c, B, f0, maxviol, R, select_tol, b.didx, b.dkey);
    HIPCHK(c, hipGetLastError());
    if (b.x) {
        HIPCHK(c, hipMemsetAsync(b.dx, 0, (size_t)B * n * 8, c->stream));
        const hipError_t qe = (hipError_t)small_gather_launch(X, n, R, B, b.didx, b.dx, c->stream);
        if (qe != hipSuccess) return launch_failed(c, name, qe);
    }
    return 0;
}

// fetch (waits for the stream, so for every copy the driver has enqueued before) and hand out
int fetch_batch_best(qcqpmi_ctx *c, const BatchBest &b, int64_t B, int64_t n) {
    std::vector<int64_t> bidx(b.wanted() ? (size_t)B * 2 : 0);
    std::vector<double> bkey(bidx.size());
    if (b.wanted()) {
        HIPCHK(c, hipMemcpyAsync(bidx.data(), b.didx, bidx.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(bkey.data(), b.dkey, bkey.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (b.x) HIPCHK(c, hipMemcpyAsync(b.x, b.dx, (size_t)B * n * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, spin_sync(c->stream));
    for (int64_t p = 0; p < B && b.wanted(); p++) {
        if (b.index) b.index[p] = bidx[(size_t)2 * p];
        if (b.f0) b.f0[p] = bkey[(size_t)2 * p];
        if (b.maxviol) b.maxviol[p] = bkey[(size_t)2 * p + 1];
    }
    return 0;
}

// the end of a call without restarts (SDR, SPECTRAL, the ADMM setup), its launch enqueued: the symmetry check, the outputs, the wait
int finish_problems(qcqpmi_ctx *c, const char *name, const BatchCall &f, const int *ticket) {
    const int rc = check_symmetric(c, name, ticket, false);
    if (rc) return rc;
    HIPCHK(c, f.download(c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

// The end of a restart call (CD, ADMM, chain), its launch enqueued: the best restart per problem is selected from f0 / maxviol / X on
// the device; the host copy of the record block is allocated NOW, while the kernels run (megabytes of fresh pages: 18.2 ms against
// 16.0 when it came after the wait, profiles/r15_small_batch_refactor.md); the first wait is the symmetry check; then the records, the
// frame's outputs (the points) and the winners come down, and the records (arrays of `count` entries) go to `out`; of the chain's last
// stage, `last_row` on, f0 / maxviol go to final_f0 / final_maxviol as well.
template <int WHICH>
int finish_restarts(qcqpmi_ctx *c, const char *name, const BatchCall &f, const BatchBest &best, const int *ticket, const double *f0, const double *maxviol,
                    const double *X, int64_t B, int64_t R, int64_t n, double select_tol, const char *records, size_t count, const RecordsOut &out,
                    size_t last_row = 0, double *final_f0 = nullptr, double *final_maxviol = nullptr) {
    int rc = select_batch_best(c, name, best, f0, maxviol, X, B, R, n, select_tol);
    if (rc) return rc;
    std::vector<char> hout(record_block_bytes<WHICH>(count));
    if ((rc = check_symmetric(c, name, ticket, (WHICH & REC_ADMM) != 0))) return rc;
    HIPCHK(c, hipMemcpyAsync(hout.data(), records, hout.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, f.download(c->stream));
    if ((rc = fetch_batch_best(c, best, B, n))) return rc;
    unpack_records<WHICH>(out, hout.data(), count, 0, count);
    RecordsOut final_rows = {};
    final_rows.f0 = final_f0; final_rows.maxviol = final_maxviol;
    unpack_records<WHICH>(final_rows, hout.data(), count, last_row, (size_t)(B * R));
    return 0;
}

// ---- coordinate descent.  cons == nullptr: the context's coefficients; else [B][m][3], per_problem set (the _pc symbol).  maxn:
// CD_SMALL_MAXN, or CD_WIDE_MAXN for qcqpmi_cd_batch_run, whose problems of more than CD_SMALL_MAXN variables run the wide kernels
int cd_small_batch(qcqpmi_ctx *c, int64_t maxn, bool per_problem, const double *cons, int64_t B, const double *P0s, const double *q0s, const double *r0s,
                   int64_t R, int generate, const double *X0, int phase1, int64_t num_iters, double viol_tol, double tol, uint64_t seed,
                   uint64_t seed_stride, uint64_t first_index, double select_tol, int64_t *sweeps1, int64_t *sweeps2,
                   int64_t *visits2, int64_t *accepted2, uint8_t *ran_phase2, int *status1, int *status2, double *f0,
                   double *maxviol, double *X, int64_t *best_index, double *best_f0, double *best_maxviol, double *best_x) {
    const char *name = "cd_small_batch_run";
    int rc = check_batch_context(c, name);
    if (rc) return rc;
    if (c->n > maxn) return fail(c, QCQPMI_EUNSUPPORTED, "cd_small_batch_run: n = %lld, the small-problem kernel takes n <= %lld (%s)", (long long)c->n, (long long)maxn,
                                 maxn > CD_SMALL_MAXN ? "two coordinates per lane" : "one lane per coordinate");
    if (B < 1 || R < 1 || num_iters < 0 || !(tol > 0.0) || !P0s || !q0s || !r0s || (!generate && !X0))
        return fail(c, QCQPMI_EINVAL, "cd_small_batch_run: bad B / R / num_iters / tol, or a missing input array");
    if ((rc = check_batch_count(c, name, B, R))) return rc;
    const int64_t m = c->m;
    if (per_problem) {
        if (!cons) return fail(c, QCQPMI_EINVAL, "cd_small_batch_run_pc: missing cons (B x m x 3 coefficients)");
        if ((rc = check_batch_cons(c, "cd_small_batch_run_pc", cons, B, m))) return rc;
        if (m == 0) cons = nullptr;       // nothing to stage: the shared kernels
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->n, T = B * R;
    CdSmallArgs a;
    BatchCall f;
    BatchBest best = {best_index, best_f0, best_maxviol, best_x};
    char *records = nullptr;
    declare_objectives(f, a, B, n, P0s, q0s, r0s);
    declare_restarts(c, f, a, best, &records, record_block_bytes<REC_CD>((size_t)T), B, R, generate, X0, X, cons, seed, seed_stride, first_index);
    HIPCHK(c, f.reserve(c->sb_work, c->stream));
    HIPCHK(c, f.upload(c->stream));
    a.phase1 = phase1 ? 1 : 0; a.num_iters = num_iters; a.viol_tol = viol_tol; a.tol = tol;
    bind_records<REC_CD>(a, records, (size_t)T);
    const int maxc = c->maxc <= 1 ? 1 : 4;
    int threads = 0;
    const int cap = cd_small_workgroups(n, maxc, cons ? m : 0, B * R, c->device, &threads);
    if (cap < 1) return occupancy_failed(c, name, cap);
    const TicketPlan plan = ticket_partition(B, R, cap, threads / 64);
    a.RC = plan.RC; a.chunks = plan.chunks;
    tic(c, 2);
    const hipError_t qe = (hipError_t)cd_small_launch(a, maxc, plan.wgs, threads, c->stream);
    toc(c, 2);
    if (qe != hipSuccess) return launch_failed(c, name, qe);
    c->last_cd2_kernel = cd_small_name(maxc, cons != nullptr, n > CD_SMALL_MAXN);
    return finish_restarts<REC_CD>(c, name, f, best, a.ticket, a.f0, a.maxviol, a.X, B, R, n, select_tol, records, (size_t)T,
                                   {sweeps1, sweeps2, visits2, accepted2, nullptr, nullptr, f0, maxviol, status1, status2, ran_phase2});
}

// ---- suggest(SDR) for problems of the unit-diagonal family that share the context's constraints x_i^2 == d_i: the relaxation (mixing
// method), its multipliers and S samples per problem.  ds == nullptr: the context's d; else [B][n], per_problem set (the _pc symbol).
// maxn: SDR_SMALL_MAXN, or SDR_WIDE_MAXN for qcqpmi_sdr_batch[_pc], whose problems of more than SDR_SMALL_MAXN variables run the wide kernel
int sdr_small_batch(qcqpmi_ctx *c, int64_t maxn, bool per_problem, const double *ds, int64_t B, const double *P0s, const double *q0s, const double *r0s,
                    int64_t S, int max_sweeps, double tol, uint64_t seed, uint64_t seed_stride, uint64_t first_index, const double *V0s,
                    double *V, double *primal, double *y, int64_t *sweeps, double *X) {
    const char *name = "sdr_small_batch";
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (c->n > maxn) return fail(c, QCQPMI_EUNSUPPORTED, "sdr_small_batch: n = %lld, the small-problem kernel takes n <= %lld (%s)", (long long)c->n, (long long)maxn,
                                 maxn > SDR_SMALL_MAXN ? "C_b packed, two coordinates per lane in the samples" : "the full C_b in LDS");
    if (!c->sep || c->unit_d.empty()) return fail(c, QCQPMI_EUNSUPPORTED, "sdr_small_batch: the constraints are not of the unit-diagonal family (every coordinate exactly one constraint p x_i^2 + r == 0 with -r / p > 0)");
    if (B < 1 || S < 0 || max_sweeps < 0 || !(tol >= 0.0) || !P0s || !q0s || !r0s)
        return fail(c, QCQPMI_EINVAL, "sdr_small_batch: bad B / S / max_sweeps / tol, or a missing input array");
    if (B >= (1LL << 30) || S >= (1LL << 30) || B * (S > 0 ? S : 1) >= (1LL << 30)) return fail(c, QCQPMI_EINVAL, "sdr_small_batch: B = %lld problems with S = %lld samples, at most 2^30 - 1 per call", (long long)B, (long long)S);
    const int64_t n = c->n, N = n + 1;
    if (per_problem) {
        if (!ds) return fail(c, QCQPMI_EINVAL, "sdr_small_batch_pc: missing ds (B x n)");
        for (int64_t k = 0; k < B * n; k++)
            if (!(ds[k] > 0.0) || !std::isfinite(ds[k]))
                return fail(c, QCQPMI_EINVAL, "sdr_small_batch_pc: d of coordinate %lld of problem %lld is not a positive finite number", (long long)(k % n), (long long)(k / n));
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t ns = ds ? B * n : n;      // entries of s
    const size_t vbytes = (size_t)B * N * SDR_SMALL_K * 8;
    std::vector<double> sv((size_t)ns);
    for (int64_t i = 0; i < ns; i++) sv[(size_t)i] = sqrt(ds ? ds[i] : c->unit_d[(size_t)i]);
    SdrSmallArgs a;
    BatchCall f;
    declare_objectives(f, a, B, n, P0s, q0s, r0s);
    f.in(sv.data(), (size_t)ns * 8, &a.s);
    f.in(V0s, vbytes, &a.V0s);
    f.out(V, vbytes, &a.V);
    f.out(primal, (size_t)B * 8, &a.primal);
    f.out(y, (size_t)B * N * 8, &a.y);
    f.out(sweeps, (size_t)B * 8, &a.sweeps);
    f.out(X, (size_t)B * S * n * 8, &a.X);      // S == 0: no room, no copy, and the kernel does not write it
    f.ticket(&a.ticket);
    HIPCHK(c, f.reserve(c->ss_work, c->stream));
    HIPCHK(c, f.upload(c->stream));
    HIPCHK(c, spin_sync(c->stream));      // sv goes out of scope; the pageable copies above have been staged
    a.n = (int)n; a.B = B; a.S = S; a.s_stride = ds ? n : 0;
    a.max_sweeps = max_sweeps; a.tol = tol; a.seed = seed; a.seed_stride = seed_stride; a.first_index = first_index;
    const int wgs = sdr_small_workgroups((int)n, B, c->device);
    if (wgs < 1) return occupancy_failed(c, name, wgs);
    const hipError_t qe = (hipError_t)sdr_small_launch(a, wgs, c->stream);
    if (qe != hipSuccess) return launch_failed(c, name, qe);
    return finish_problems(c, name, f, a.ticket);
}

// ---- suggest(SPECTRAL) for problems whose constraints aggregate to ONE sphere (relop_eq) or ONE ball: agg = [a (n) | beta (n) | gamma]
// per problem (agg_stride = 2 n + 1) or shared (agg_stride = 0).  The context gives n, the device and the buffer; its constraints are not read.
// maxn: SPECTRAL_SMALL_MAXN, or SPECTRAL_WIDE_MAXN for qcqpmi_spectral_batch, whose problems of more than SPECTRAL_SMALL_MAXN variables run the wide kernel
int spectral_small_batch(qcqpmi_ctx *c, int64_t maxn, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *agg, int64_t agg_stride,
                         int relop_eq, int max_sweeps, double tol, double *x, double *bound, double *mu, double *lam, int64_t *sweeps,
                         int *branch, int *status) {
    const char *name = "spectral_small_batch";
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (c->n > maxn) return fail(c, QCQPMI_EUNSUPPORTED, "spectral_small_batch: n = %lld, the small-problem kernel takes n <= %lld (%s)", (long long)c->n, (long long)maxn,
                                 maxn > SPECTRAL_SMALL_MAXN ? "one array G_b in LDS, two eigenvalues per lane" : "A_b and Q_b in LDS, one lane per eigenvalue");
    const int64_t n = c->n, na = 2 * n + 1;
    if (B < 1 || B >= (1LL << 30) || max_sweeps < 0 || !(tol >= 0.0) || !P0s || !q0s || !r0s || !agg || (agg_stride != 0 && agg_stride != na))
        return fail(c, QCQPMI_EINVAL, "spectral_small_batch: bad B / max_sweeps / tol / agg_stride (0 or 2 n + 1), or a missing input array");
    const int64_t nagg = agg_stride ? B : 1;
    for (int64_t b = 0; b < nagg; b++) {
        const double *ab = agg + b * na;
        double r2 = -ab[2 * n];
        for (int64_t i = 0; i < n; i++) {
            if (!(ab[i] > 0.0) || !std::isfinite(ab[i]) || !std::isfinite(ab[n + i]))
                return fail(c, QCQPMI_EINVAL, "spectral_small_batch: a = %g, beta = %g of coordinate %lld of problem %lld: a must be positive, both finite", ab[i], ab[n + i], (long long)i, (long long)b);
            r2 += ab[n + i] * ab[n + i] / (4.0 * ab[i]);
        }
        if (!(r2 > 0.0) || !std::isfinite(r2))
            return fail(c, QCQPMI_EINVAL, "spectral_small_batch: rho^2 = sum beta^2 / (4 a) - gamma = %g of problem %lld is not positive and finite", r2, (long long)b);
    }
    HIPCHK(c, hipSetDevice(c->device));
    SpectralSmallArgs a;
    BatchCall f;
    declare_objectives(f, a, B, n, P0s, q0s, r0s);
    f.in(agg, (size_t)nagg * na * 8, &a.agg);
    f.out(x, (size_t)B * n * 8, &a.x);
    const int ilam = f.room((size_t)B * n * 8, &a.lam);      // lies behind x, comes down behind mu
    f.out(bound, (size_t)B * 8, &a.bound);
    f.out(mu, (size_t)B * 8, &a.mu);
    f.fetch(ilam, lam);
    f.out(sweeps, (size_t)B * 8, &a.sweeps);
    f.out(branch, (size_t)B * 4, &a.branch);
    f.out(status, (size_t)B * 4, &a.status);
    f.ticket(&a.ticket);
    HIPCHK(c, f.reserve(c->ss_work, c->stream));
    HIPCHK(c, f.upload(c->stream));
    a.n = (int)n; a.B = B; a.agg_stride = agg_stride;
    a.relop_eq = relop_eq ? 1 : 0; a.max_sweeps = max_sweeps; a.tol = tol;
    const bool wide = n > SPECTRAL_SMALL_MAXN;
    const int wgs = wide ? spectral_wide_workgroups((int)n, B, c->device) : spectral_small_workgroups((int)n, B, c->device);
    if (wgs < 1) return occupancy_failed(c, name, wgs);
    const hipError_t qe = (hipError_t)(wide ? spectral_wide_launch(a, wgs, c->stream) : spectral_small_launch(a, wgs, c->stream));
    if (qe != hipSuccess) return launch_failed(c, name, qe);
    return finish_problems(c, name, f, a.ticket);
}

// ---- improve(ADMM), R restarts each (admm_small.h); qcqpmi_last_cd_kernel is not touched either.  maxn: ADMM_SMALL_MAXN, or ADMM_WIDE_MAXN
// for qcqpmi_admm_batch_run, whose problems of more than ADMM_SMALL_MAXN variables run the wide kernels
int admm_small_batch(qcqpmi_ctx *c, int64_t maxn, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *cons,
                     const double *rhos, const double *Minvs, int64_t R, int generate, const double *X0, int phase1,
                     int64_t num_iters, double tol, double viol_lim, uint64_t seed, uint64_t seed_stride, uint64_t first_index,
                     double select_tol, int64_t *iters1, int64_t *iters2, double *f0, double *maxviol, double *X,
                     int64_t *best_index, double *best_f0, double *best_maxviol, double *best_x) {
    const char *name = "admm_small_batch_run";
    int rc = check_batch_context(c, name);
    if (rc) return rc;
    if (c->n > maxn) return fail(c, QCQPMI_EUNSUPPORTED, "admm_small_batch_run: n = %lld, the small-problem kernel takes n <= %lld (%s)", (long long)c->n, (long long)maxn,
                                 maxn > ADMM_SMALL_MAXN ? "two coordinates per lane" : "one lane per coordinate");
    if (B < 1 || R < 1 || num_iters < 0 || !P0s || !q0s || !r0s || !rhos || !Minvs || (!generate && !X0))
        return fail(c, QCQPMI_EINVAL, "admm_small_batch_run: bad B / R / num_iters, or a missing input array");
    if ((rc = check_batch_count(c, name, B, R))) return rc;
    const int64_t m = c->m;
    if (m < 1) return fail(c, QCQPMI_EINVAL, "admm_small_batch_run: the context has no constraint (the consensus average divides by m)");
    if ((rc = check_batch_rhos(c, name, rhos, B))) return rc;
    if (cons && (rc = check_batch_cons(c, name, cons, B, m))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->n, T = B * R;
    AdmmSmallArgs a;
    BatchCall f;
    BatchBest best = {best_index, best_f0, best_maxviol, best_x};
    char *records = nullptr;
    declare_objectives(f, a, B, n, P0s, q0s, r0s, Minvs, &a.Minvs);
    f.in(rhos, (size_t)B * 8, &a.rhos);
    declare_restarts(c, f, a, best, &records, record_block_bytes<REC_ADMM>((size_t)T), B, R, generate, X0, X, cons, seed, seed_stride, first_index);
    HIPCHK(c, f.reserve(c->sb_work, c->stream));
    HIPCHK(c, f.upload(c->stream));
    a.phase1 = phase1 ? 1 : 0; a.num_iters = num_iters; a.tol = tol; a.viol_lim = viol_lim;
    bind_records<REC_ADMM>(a, records, (size_t)T);
    const int maxc = c->maxc <= 1 ? 1 : 4;
    int threads = 0;
    const int cap = admm_small_workgroups(n, maxc, cons ? m : 0, B * R, c->device, &threads);
    if (cap < 1) return occupancy_failed(c, name, cap);
    const TicketPlan plan = ticket_partition(B, R, cap, threads / 64);      // workgroups of four waves; four or eight in the wide kernels
    a.RC = plan.RC; a.chunks = plan.chunks;
    const hipError_t qe = (hipError_t)admm_small_launch(a, maxc, plan.wgs, threads, c->stream);
    if (qe != hipSuccess) return launch_failed(c, name, qe);
    c->last_admm_kernel = admm_small_name(maxc, cons != nullptr, n > ADMM_SMALL_MAXN);
    c->last_admm_C = 0;
    return finish_restarts<REC_ADMM>(c, name, f, best, a.ticket, a.f0, a.maxviol, a.X, B, R, n, select_tol, records, (size_t)T,
                                     {nullptr, nullptr, nullptr, nullptr, iters1, iters2, f0, maxviol, nullptr, nullptr, nullptr});
}

// ---- improve([method, ...]): up to CHAIN_MAX_STAGES stages of CD or ADMM one after the other in ONE launch (chain_small.h).  The
// per-stage records live in one block of the work buffer (restart_records, batch_call.h: the CD and the ADMM arrays, 73 bytes per stage
// and restart), every array [nstages][B R] and zeroed before the launch.  The final f0 / maxviol are the last stage's rows.
int chain_small_batch(qcqpmi_ctx *c, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *cons, const double *rhos,
                      const double *Minvs, int64_t R, int generate, const double *X0, int nstages, const qcqpmi_chain_stage *stages, uint64_t seed,
                      uint64_t seed_stride, uint64_t first_index, double select_tol, int64_t *st_sweeps1, int64_t *st_sweeps2,
                      int64_t *st_visits2, int64_t *st_accepted2, uint8_t *st_ran_phase2, int *st_status1, int *st_status2,
                      int64_t *st_iters1, int64_t *st_iters2, double *st_f0, double *st_maxviol, double *f0, double *maxviol, double *X,
                      int64_t *best_index, double *best_f0, double *best_maxviol, double *best_x) {
    const char *name = "chain_small_batch_run";
    int rc = check_batch_context(c, name);
    if (rc) return rc;
    if (c->n > CHAIN_SMALL_MAXN) return fail(c, QCQPMI_EUNSUPPORTED, "chain_small_batch_run: n = %lld, the chain kernel takes n <= %lld (one lane per coordinate)", (long long)c->n,
                                             (long long)CHAIN_SMALL_MAXN);
    if (nstages < 1 || nstages > CHAIN_MAX_STAGES || !stages)
        return fail(c, QCQPMI_EINVAL, "chain_small_batch_run: nstages = %d, 1 to %d stages per launch (and their descriptors)", nstages, CHAIN_MAX_STAGES);
    if (B < 1 || R < 1 || !P0s || !q0s || !r0s || (!generate && !X0)) return fail(c, QCQPMI_EINVAL, "chain_small_batch_run: bad B / R, or a missing input array");
    bool any_admm = false;
    for (int s = 0; s < nstages; s++) {
        const qcqpmi_chain_stage &g = stages[s];
        if (g.method != CHAIN_CD && g.method != CHAIN_ADMM) return fail(c, QCQPMI_EINVAL, "chain_small_batch_run: stage %d has method %d (0: COORD_DESCENT, 1: ADMM)", s, g.method);
        if (g.num_iters < 0 || (g.method == CHAIN_CD && !(g.tol > 0.0))) return fail(c, QCQPMI_EINVAL, "chain_small_batch_run: stage %d has a bad num_iters / tol", s);
        any_admm = any_admm || g.method == CHAIN_ADMM;
    }
    if ((rc = check_batch_count(c, name, B, R))) return rc;
    const int64_t m = c->m;
    if (any_admm) {
        if (!rhos || !Minvs) return fail(c, QCQPMI_EINVAL, "chain_small_batch_run: an ADMM stage needs rhos and Minvs");
        if (m < 1) return fail(c, QCQPMI_EINVAL, "chain_small_batch_run: the context has no constraint (the consensus average of an ADMM stage divides by m)");
        if ((rc = check_batch_rhos(c, name, rhos, B))) return rc;
    }
    if (cons && (rc = check_batch_cons(c, name, cons, B, m))) return rc;
    if (m == 0) cons = nullptr;       // nothing to stage: the shared kernels
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->n, T = B * R, ST = (int64_t)nstages * T;
    const size_t record_bytes = record_block_bytes<REC_CD | REC_ADMM>((size_t)ST);
    ChainSmallArgs a;
    BatchCall f;
    BatchBest best = {best_index, best_f0, best_maxviol, best_x};
    char *records = nullptr;
    declare_objectives(f, a, B, n, P0s, q0s, r0s, any_admm ? Minvs : nullptr, &a.Minvs);
    f.in(any_admm ? rhos : nullptr, (size_t)B * 8, &a.rhos);
    declare_restarts(c, f, a, best, &records, record_bytes, B, R, generate, X0, X, cons, seed, seed_stride, first_index);
    HIPCHK(c, f.reserve(c->sb_work, c->stream));
    HIPCHK(c, f.upload(c->stream));
    HIPCHK(c, hipMemsetAsync(records, 0, record_bytes, c->stream));      // what a stage does not produce stays zero
    a.nstages = nstages;
    for (int s = 0; s < CHAIN_MAX_STAGES; s++) {
        ChainStage &g = a.st[s];
        memset(&g, 0, sizeof(g));
        if (s >= nstages) continue;
        g.method = stages[s].method; g.phase1 = stages[s].phase1 ? 1 : 0; g.num_iters = stages[s].num_iters;
        g.tol = stages[s].tol; g.viol_tol = stages[s].viol_tol; g.viol_lim = stages[s].viol_lim;
        bind_records<REC_CD | REC_ADMM>(g, records, (size_t)T, (size_t)nstages, (size_t)s);
    }
    const int maxc = c->maxc <= 1 ? 1 : 4;
    const int cap = chain_small_workgroups(n, maxc, cons ? m : 0, B * R, c->device);
    if (cap < 1) return occupancy_failed(c, name, cap);
    const TicketPlan plan = ticket_partition(B, R, cap, 4);      // workgroups of four waves
    a.RC = plan.RC; a.chunks = plan.chunks;
    tic(c, 2);
    const hipError_t qe = (hipError_t)chain_small_launch(a, maxc, plan.wgs, c->stream);
    toc(c, 2);
    if (qe != hipSuccess) return launch_failed(c, name, qe);
    c->last_cd2_kernel = chain_small_name(maxc, cons != nullptr);
    const ChainStage &last = a.st[nstages - 1];
    return finish_restarts<REC_CD | REC_ADMM>(
        c, name, f, best, a.ticket, last.f0, last.maxviol, a.X, B, R, n, select_tol, records, (size_t)ST,
        {st_sweeps1, st_sweeps2, st_visits2, st_accepted2, st_iters1, st_iters2, st_f0, st_maxviol, st_status1, st_status2, st_ran_phase2},
        (size_t)(nstages - 1) * T, f0, maxviol);
}

// ---- the setup of improve(ADMM) on the device (admm_setup.h): rho_b by the reference's rule (rho == nullptr) or the caller's, and
// Minv_b = (2 (P0_b + rho_b m I))^-1, both from one eigendecomposition per problem.  n <= ADMM_SETUP_SMALL_MAXN runs the narrow kernel
int admm_setup_batch(qcqpmi_ctx *c, int64_t B, const double *P0s, const double *rho, int max_sweeps, double tol, double *rhos, double *lambda_min,
                     double *Minvs, int64_t *sweeps, int *status) {
    const char *name = "admm_batch_setup";
    int rc = check_batch_context(c, name);
    if (rc) return rc;
    if (c->n > ADMM_SETUP_MAXN) return fail(c, QCQPMI_EUNSUPPORTED, "admm_batch_setup: n = %lld, the setup kernels take n <= %lld (one array G_b in LDS, two eigenvalues per lane)",
                                            (long long)c->n, (long long)ADMM_SETUP_MAXN);
    if (B < 1 || B >= (1LL << 30)) return fail(c, QCQPMI_EINVAL, "admm_batch_setup: B = %lld problems, 1 to 2^30 - 1 per call", (long long)B);
    if (!P0s) return fail(c, QCQPMI_EINVAL, "admm_batch_setup: the objective matrices P0s are missing");
    if (max_sweeps < 1) return fail(c, QCQPMI_EINVAL, "admm_batch_setup: max_sweeps = %d, at least one sweep", max_sweeps);
    if (!(tol > 0.0) || !std::isfinite(tol)) return fail(c, QCQPMI_EINVAL, "admm_batch_setup: tol = %g is not positive and finite", tol);
    if (rho && (!(*rho > 0.0) || !std::isfinite(*rho))) return fail(c, QCQPMI_EINVAL, "admm_batch_setup: rho = %g is not positive and finite", *rho);
    const int64_t n = c->n, m = c->m;
    if (m < 1) return fail(c, QCQPMI_EINVAL, "admm_batch_setup: the context has no constraint (the rule divides by m)");
    HIPCHK(c, hipSetDevice(c->device));
    AdmmSetupArgs a;
    BatchCall f;
    f.in(P0s, (size_t)B * n * n * 8, &a.P0s);
    const int iM = f.room((size_t)B * n * n * 8, &a.Minvs);      // lies behind P0s, comes down behind lambda_min
    f.out(rhos, (size_t)B * 8, &a.rhos);
    f.out(lambda_min, (size_t)B * 8, &a.lambda_min);
    f.fetch(iM, Minvs);
    f.out(sweeps, (size_t)B * 8, &a.sweeps);
    f.out(status, (size_t)B * 4, &a.status);
    f.ticket(&a.ticket);
    HIPCHK(c, f.reserve(c->ss_work, c->stream));
    HIPCHK(c, f.upload(c->stream));
    if (rho) HIPCHK(c, hipMemsetAsync(a.Minvs, 0, (size_t)B * n * n * 8, c->stream));      // a problem of status 3 is not written
    a.n = (int)n; a.B = B;
    a.m = (double)m; a.has_rho = rho ? 1 : 0; a.rho = rho ? *rho : 0.0;
    a.max_sweeps = max_sweeps; a.tol = tol;
    const int wgs = admm_setup_workgroups((int)n, B, c->device);
    if (wgs < 1) return occupancy_failed(c, name, wgs);
    const hipError_t qe = (hipError_t)admm_setup_launch(a, wgs, c->stream);
    if (qe != hipSuccess) return launch_failed(c, name, qe);
    return finish_problems(c, name, f, a.ticket);
}

}  // namespace


extern "C" {

int qcqpmi_cd_small_batch_run(qcqpmi_ctx *c, int64_t B, const double *P0s, const double *q0s, const double *r0s, int64_t R, int generate,
                              const double *X0, int phase1, int64_t num_iters, double viol_tol, double tol, uint64_t seed,
                              uint64_t seed_stride, uint64_t first_index, double select_tol, int64_t *sweeps1, int64_t *sweeps2,
                              int64_t *visits2, int64_t *accepted2, uint8_t *ran_phase2, int *status1, int *status2, double *f0,
                              double *maxviol, double *X, int64_t *best_index, double *best_f0, double *best_maxviol, double *best_x) {
    return cd_small_batch(c, CD_SMALL_MAXN, false, nullptr, B, P0s, q0s, r0s, R, generate, X0, phase1, num_iters, viol_tol, tol, seed, seed_stride, first_index,
                          select_tol, sweeps1, sweeps2, visits2, accepted2, ran_phase2, status1, status2, f0, maxviol, X, best_index, best_f0,
                          best_maxviol, best_x);
}

// ---- the same launch with PER-PROBLEM constraint coefficients cons [B][m][3]: the context fixes the structure (cd_small.h)
int qcqpmi_cd_small_batch_run_pc(qcqpmi_ctx *c, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *cons,
                                 int64_t R, int generate, const double *X0, int phase1, int64_t num_iters, double viol_tol, double tol,
                                 uint64_t seed, uint64_t seed_stride, uint64_t first_index, double select_tol, int64_t *sweeps1,
                                 int64_t *sweeps2, int64_t *visits2, int64_t *accepted2, uint8_t *ran_phase2, int *status1, int *status2,
                                 double *f0, double *maxviol, double *X, int64_t *best_index, double *best_f0, double *best_maxviol,
                                 double *best_x) {
    return cd_small_batch(c, CD_SMALL_MAXN, true, cons, B, P0s, q0s, r0s, R, generate, X0, phase1, num_iters, viol_tol, tol, seed, seed_stride, first_index,
                          select_tol, sweeps1, sweeps2, visits2, accepted2, ran_phase2, status1, status2, f0, maxviol, X, best_index, best_f0,
                          best_maxviol, best_x);
}

// ---- the batch for 1 <= n <= 128: the two symbols above for n <= 64 (cons == NULL: shared constraints), the wide kernels past it
int qcqpmi_cd_batch_run(qcqpmi_ctx *c, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *cons, int64_t R,
                        int generate, const double *X0, int phase1, int64_t num_iters, double viol_tol, double tol, uint64_t seed,
                        uint64_t seed_stride, uint64_t first_index, double select_tol, int64_t *sweeps1, int64_t *sweeps2, int64_t *visits2,
                        int64_t *accepted2, uint8_t *ran_phase2, int *status1, int *status2, double *f0, double *maxviol, double *X,
                        int64_t *best_index, double *best_f0, double *best_maxviol, double *best_x) {
    return cd_small_batch(c, CD_WIDE_MAXN, cons != nullptr, cons, B, P0s, q0s, r0s, R, generate, X0, phase1, num_iters, viol_tol, tol, seed, seed_stride,
                          first_index, select_tol, sweeps1, sweeps2, visits2, accepted2, ran_phase2, status1, status2, f0, maxviol, X, best_index,
                          best_f0, best_maxviol, best_x);
}

// ---- improve(ADMM) for B small problems (n <= 64), R restarts each (admm_small.h)
int qcqpmi_admm_small_batch_run(qcqpmi_ctx *c, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *cons,
                                const double *rhos, const double *Minvs, int64_t R, int generate, const double *X0, int phase1,
                                int64_t num_iters, double tol, double viol_lim, uint64_t seed, uint64_t seed_stride, uint64_t first_index,
                                double select_tol, int64_t *iters1, int64_t *iters2, double *f0, double *maxviol, double *X,
                                int64_t *best_index, double *best_f0, double *best_maxviol, double *best_x) {
    return admm_small_batch(c, ADMM_SMALL_MAXN, B, P0s, q0s, r0s, cons, rhos, Minvs, R, generate, X0, phase1, num_iters, tol, viol_lim, seed, seed_stride,
                            first_index, select_tol, iters1, iters2, f0, maxviol, X, best_index, best_f0, best_maxviol, best_x);
}

// ---- the same for 1 <= n <= 128: the launch above for n <= 64, the wide kernels past it
int qcqpmi_admm_batch_run(qcqpmi_ctx *c, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *cons,
                          const double *rhos, const double *Minvs, int64_t R, int generate, const double *X0, int phase1, int64_t num_iters,
                          double tol, double viol_lim, uint64_t seed, uint64_t seed_stride, uint64_t first_index, double select_tol,
                          int64_t *iters1, int64_t *iters2, double *f0, double *maxviol, double *X, int64_t *best_index, double *best_f0,
                          double *best_maxviol, double *best_x) {
    return admm_small_batch(c, ADMM_WIDE_MAXN, B, P0s, q0s, r0s, cons, rhos, Minvs, R, generate, X0, phase1, num_iters, tol, viol_lim, seed, seed_stride,
                            first_index, select_tol, iters1, iters2, f0, maxviol, X, best_index, best_f0, best_maxviol, best_x);
}

// ---- improve([method, ...]) for B small problems (n <= 64): up to four stages of CD or ADMM in one launch (chain_small.h)
int qcqpmi_chain_small_batch_run(qcqpmi_ctx *c, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *cons,
                                 const double *rhos, const double *Minvs, int64_t R, int generate, const double *X0, int nstages,
                                 const qcqpmi_chain_stage *stages, uint64_t seed, uint64_t seed_stride, uint64_t first_index,
                                 double select_tol, int64_t *st_sweeps1, int64_t *st_sweeps2, int64_t *st_visits2, int64_t *st_accepted2,
                                 uint8_t *st_ran_phase2, int *st_status1, int *st_status2, int64_t *st_iters1, int64_t *st_iters2,
                                 double *st_f0, double *st_maxviol, double *f0, double *maxviol, double *X, int64_t *best_index,
                                 double *best_f0, double *best_maxviol, double *best_x) {
    return chain_small_batch(c, B, P0s, q0s, r0s, cons, rhos, Minvs, R, generate, X0, nstages, stages, seed, seed_stride, first_index, select_tol,
                             st_sweeps1, st_sweeps2, st_visits2, st_accepted2, st_ran_phase2, st_status1, st_status2, st_iters1, st_iters2,
                             st_f0, st_maxviol, f0, maxviol, X, best_index, best_f0, best_maxviol, best_x);
}

// ---- rhos and Minvs of the two calls above from one eigendecomposition per problem on the device (admm_setup.h), 1 <= n <= 128
int qcqpmi_admm_batch_setup(qcqpmi_ctx *c, int64_t B, const double *P0s, const double *rho, int max_sweeps, double tol, double *rhos,
                            double *lambda_min, double *Minvs, int64_t *sweeps, int *status) {
    return admm_setup_batch(c, B, P0s, rho, max_sweeps, tol, rhos, lambda_min, Minvs, sweeps, status);
}

int qcqpmi_sdr_small_batch(qcqpmi_ctx *c, int64_t B, const double *P0s, const double *q0s, const double *r0s, int64_t S, int max_sweeps,
                           double tol, uint64_t seed, uint64_t seed_stride, uint64_t first_index, const double *V0s, double *V,
                           double *primal, double *y, int64_t *sweeps, double *X) {
    return sdr_small_batch(c, SDR_SMALL_MAXN, false, nullptr, B, P0s, q0s, r0s, S, max_sweeps, tol, seed, seed_stride, first_index, V0s, V, primal, y, sweeps, X);
}

// ---- the same launch with PER-PROBLEM d: ds [B][n] replaces the context's d problem by problem (the context must still be of the family)
int qcqpmi_sdr_small_batch_pc(qcqpmi_ctx *c, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *ds, int64_t S,
                              int max_sweeps, double tol, uint64_t seed, uint64_t seed_stride, uint64_t first_index, const double *V0s,
                              double *V, double *primal, double *y, int64_t *sweeps, double *X) {
    return sdr_small_batch(c, SDR_SMALL_MAXN, true, ds, B, P0s, q0s, r0s, S, max_sweeps, tol, seed, seed_stride, first_index, V0s, V, primal, y, sweeps, X);
}

// ---- the same two for 1 <= n <= 128: the launches above for n <= 64, the wide kernel (sdr_small_kernel<true>) past it
int qcqpmi_sdr_batch(qcqpmi_ctx *c, int64_t B, const double *P0s, const double *q0s, const double *r0s, int64_t S, int max_sweeps, double tol,
                     uint64_t seed, uint64_t seed_stride, uint64_t first_index, const double *V0s, double *V, double *primal, double *y,
                     int64_t *sweeps, double *X) {
    return sdr_small_batch(c, SDR_WIDE_MAXN, false, nullptr, B, P0s, q0s, r0s, S, max_sweeps, tol, seed, seed_stride, first_index, V0s, V, primal, y, sweeps, X);
}

int qcqpmi_sdr_batch_pc(qcqpmi_ctx *c, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *ds, int64_t S,
                        int max_sweeps, double tol, uint64_t seed, uint64_t seed_stride, uint64_t first_index, const double *V0s, double *V,
                        double *primal, double *y, int64_t *sweeps, double *X) {
    return sdr_small_batch(c, SDR_WIDE_MAXN, true, ds, B, P0s, q0s, r0s, S, max_sweeps, tol, seed, seed_stride, first_index, V0s, V, primal, y, sweeps, X);
}

// ---- suggest(SPECTRAL) for B small problems (n <= 64) whose constraints aggregate to one sphere or one ball (spectral_small.h)
int qcqpmi_spectral_small_batch(qcqpmi_ctx *c, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *agg,
                                int64_t agg_stride, int relop_eq, int max_sweeps, double tol, double *x, double *bound, double *mu, double *lam,
                                int64_t *sweeps, int *branch, int *status) {
    return spectral_small_batch(c, SPECTRAL_SMALL_MAXN, B, P0s, q0s, r0s, agg, agg_stride, relop_eq, max_sweeps, tol, x, bound, mu, lam, sweeps, branch, status);
}

// ---- the same for 1 <= n <= 128: the launch above for n <= 64, the wide kernel (spectral_wide_kernel, spectral_wide.h) past it
int qcqpmi_spectral_batch(qcqpmi_ctx *c, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *agg, int64_t agg_stride,
                          int relop_eq, int max_sweeps, double tol, double *x, double *bound, double *mu, double *lam, int64_t *sweeps, int *branch,
                          int *status) {
    return spectral_small_batch(c, SPECTRAL_WIDE_MAXN, B, P0s, q0s, r0s, agg, agg_stride, relop_eq, max_sweeps, tol, x, bound, mu, lam, sweeps, branch, status);
}

}  // extern "C"
