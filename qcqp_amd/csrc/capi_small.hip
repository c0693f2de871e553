// Small-problem batch part of the C ABI: B small problems over the context's constraint structure in ONE
// persistent launch of cd_small.hip, admm_small.hip, chain_small.hip, sdr_small.hip or spectral_small.hip (narrow and wide kernel; the ADMM setup kernels live there too).  A call works in a device buffer of its own
// (sb_work for CD and ADMM, ss_work for SDR, SPECTRAL and the ADMM setup): the resident population, its evaluation, its status codes and an installed ADMM basis are not touched,
// whether the call succeeds or is refused.  The shared steps come first; a driver is its argument struct, its launch and its outputs.
// Host code only: the launcher headers, and the launch of the core's selection kernel through capi_ctx.h.
#include <cmath>
#include <cstring>

#include "capi_ctx.h"
#include "cd_small.h"
#include "admm_small.h"
#include "chain_small.h"
#include "sdr_small.h"
#include "spectral_small.h"
#include "spectral_wide.h"
#include "admm_setup.h"

using namespace qcqpmi;

namespace {

// offsets into a work buffer, every piece 256-byte aligned
struct Carve {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; }
};

// host -> work buffer; a missing array or an empty piece is skipped
int stage_in(qcqpmi_ctx *c, void *dst, const void *src, size_t bytes) {
    if (src && bytes) HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    return 0;
}

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

// Tickets of a launch over B problems with R restarts each on `wgs` resident workgroups of `waves` wavefronts: whole problems when
// there are enough of them to fill the device, else chunks of RC consecutive restarts, at least one restart per wave of a workgroup.
struct TicketPlan { int64_t RC, chunks; int wgs; };      // restarts per ticket, tickets per problem, workgroups (at most one per ticket)

TicketPlan ticket_partition(int64_t B, int64_t R, int wgs, int64_t waves) {
    int64_t chunks = B >= wgs ? 1 : (wgs + B - 1) / B;
    if (chunks > (R + waves - 1) / waves) chunks = (R + waves - 1) / waves;
    TicketPlan t;
    t.RC = (R + chunks - 1) / chunks;
    t.chunks = (R + t.RC - 1) / t.RC;
    t.wgs = wgs > B * t.chunks ? (int)(B * t.chunks) : wgs;
    return t;
}

// waits for the launch that has just been enqueued and fails with `what` if its ticket[1] is set: a matrix was not symmetric
int check_symmetric(qcqpmi_ctx *c, const char *ticket, const char *what) {
    int flags[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(flags, ticket, sizeof(flags), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return flags[1] ? fail(c, QCQPMI_EINVAL, "%s", what) : 0;
}

// The best restart of every problem (QCQPForm.better folded over its R restarts, ties -> lowest index): where its pieces lie in the
// work buffer w, and where the caller wants them (any pointer may be null; none: nothing runs)
struct BatchBest {
    size_t oidx, okey, ox;       // [B][2] int64, [B][2] double, [B][n] double
    int64_t *index;
    double *f0, *maxviol, *x;
    bool wanted() const { return index || f0 || maxviol || x; }
};

// enqueue: one workgroup per problem selects, then one gather of the winners' points
int select_batch_best(qcqpmi_ctx *c, const char *name, char *w, const BatchBest &b, const double *f0, const double *maxviol, const double *X,
                      int64_t B, int64_t R, int64_t n, double select_tol) {
    if (!b.wanted()) return 0;
    launch_select_best(c, B, f0, maxviol, R, select_tol, (int64_t *)(w + b.oidx), (double *)(w + b.okey));
    HIPCHK(c, hipGetLastError());
    if (b.x) {
        HIPCHK(c, hipMemsetAsync(w + b.ox, 0, (size_t)B * n * 8, c->stream));
        const hipError_t qe = (hipError_t)small_gather_launch(X, n, R, B, (const int64_t *)(w + b.oidx), (double *)(w + b.ox), c->stream);
        if (qe != hipSuccess) return fail(c, QCQPMI_EHIP, "%s: %s", name, hipGetErrorString(qe));
    }
    return 0;
}

// fetch (waits for the stream, so for every copy the driver has enqueued before) and hand out
int fetch_batch_best(qcqpmi_ctx *c, const char *w, const BatchBest &b, int64_t B, int64_t n) {
    std::vector<int64_t> bidx(b.wanted() ? (size_t)B * 2 : 0);
    std::vector<double> bkey(bidx.size());
    if (b.wanted()) {
        HIPCHK(c, hipMemcpyAsync(bidx.data(), w + b.oidx, bidx.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(bkey.data(), w + b.okey, bkey.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (b.x) HIPCHK(c, hipMemcpyAsync(b.x, w + b.ox, (size_t)B * n * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, spin_sync(c->stream));
    for (int64_t p = 0; p < B && b.wanted(); p++) {
        if (b.index) b.index[p] = bidx[(size_t)2 * p];
        if (b.f0) b.f0[p] = bkey[(size_t)2 * p];
        if (b.maxviol) b.maxviol[p] = bkey[(size_t)2 * p + 1];
    }
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
    Carve cv;
    const size_t oP = cv.take((size_t)B * n * n * 8), oq = cv.take((size_t)B * n * 8), or0 = cv.take((size_t)B * 8);
    const size_t oX0 = cv.take(generate ? 0 : (size_t)T * n * 8), oX = cv.take((size_t)T * n * 8);
    const size_t oout = cv.take((size_t)T * 57);      // 4 x int64, 2 x double, 2 x int, 1 x uint8 per restart, array after array
    const size_t oticket = cv.take(2 * sizeof(int));
    const BatchBest best = {cv.take((size_t)B * 2 * sizeof(int64_t)), cv.take((size_t)B * 2 * sizeof(double)), cv.take((size_t)B * n * 8),
                            best_index, best_f0, best_maxviol, best_x};
    const size_t ocons = cv.take(cons ? (size_t)B * m * 24 : 0);
    HIPCHK(c, c->sb_work.reserve(c->stream, cv.off, false));
    char *w = c->sb_work;
    if ((rc = stage_in(c, w + oP, P0s, (size_t)B * n * n * 8)) || (rc = stage_in(c, w + oq, q0s, (size_t)B * n * 8)) ||
        (rc = stage_in(c, w + or0, r0s, (size_t)B * 8)) || (rc = stage_in(c, w + oX0, generate ? nullptr : X0, (size_t)T * n * 8)) ||
        (rc = stage_in(c, w + ocons, cons, (size_t)B * m * 24)))
        return rc;
    HIPCHK(c, hipMemsetAsync(w + oticket, 0, 2 * sizeof(int), c->stream));
    CdSmallArgs a;
    a.P = c->dp; a.B = B; a.R = R;
    a.P0s = (const double *)(w + oP); a.q0s = (const double *)(w + oq); a.r0s = (const double *)(w + or0);
    a.X0 = generate ? nullptr : (const double *)(w + oX0);
    a.cons = cons ? (const double *)(w + ocons) : nullptr;
    a.generate = generate ? 1 : 0; a.phase1 = phase1 ? 1 : 0; a.num_iters = num_iters; a.viol_tol = viol_tol; a.tol = tol;
    a.seed = seed; a.seed_stride = seed_stride; a.first_index = first_index;
    a.ticket = (int *)(w + oticket);
    char *o = w + oout;
    a.sweeps1 = (int64_t *)o; a.sweeps2 = (int64_t *)(o + 8 * T); a.visits2 = (int64_t *)(o + 16 * T); a.accepted2 = (int64_t *)(o + 24 * T);
    a.f0 = (double *)(o + 32 * T); a.maxviol = (double *)(o + 40 * T);
    a.status1 = (int *)(o + 48 * T); a.status2 = (int *)(o + 52 * T); a.ran2 = (uint8_t *)(o + 56 * T);
    a.X = (double *)(w + oX);
    const int maxc = c->maxc <= 1 ? 1 : 4;
    int threads = 0;
    const int cap = cd_small_workgroups(n, maxc, cons ? m : 0, B * R, c->device, &threads);
    if (cap < 1) return fail(c, QCQPMI_EHIP, "cd_small_batch_run: occupancy query failed: %s", hipGetErrorString((hipError_t)(-cap)));
    const TicketPlan plan = ticket_partition(B, R, cap, threads / 64);
    a.RC = plan.RC; a.chunks = plan.chunks;
    (void)hipEventRecord(c->timers[2].beg, c->stream);
    const hipError_t qe = (hipError_t)cd_small_launch(a, maxc, plan.wgs, threads, c->stream);
    (void)hipEventRecord(c->timers[2].end, c->stream);
    c->timers[2].valid = true;
    if (qe != hipSuccess) return fail(c, QCQPMI_EHIP, "cd_small_batch_run: %s", hipGetErrorString(qe));
    c->last_cd2_kernel = cd_small_name(maxc, cons != nullptr, n > CD_SMALL_MAXN);
    if ((rc = select_batch_best(c, name, w, best, a.f0, a.maxviol, a.X, B, R, n, select_tol))) return rc;
    std::vector<char> hout((size_t)T * 57);      // (megabytes of fresh pages: touched while the kernel runs)
    if ((rc = check_symmetric(c, w + oticket, "cd_small_batch_run: an objective matrix P0_b is not symmetric (or holds a NaN)"))) return rc;
    HIPCHK(c, hipMemcpyAsync(hout.data(), o, hout.size(), hipMemcpyDeviceToHost, c->stream));
    if (X) HIPCHK(c, hipMemcpyAsync(X, a.X, (size_t)T * n * 8, hipMemcpyDeviceToHost, c->stream));
    if ((rc = fetch_batch_best(c, w, best, B, n))) return rc;
    const char *h = hout.data();
    const size_t n8 = (size_t)T * 8;
    void *const wide[6] = {sweeps1, sweeps2, visits2, accepted2, f0, maxviol};
    for (size_t k = 0; k < 6; k++) if (wide[k]) memcpy(wide[k], h + k * n8, n8);
    if (status1) memcpy(status1, h + 6 * n8, (size_t)T * 4);
    if (status2) memcpy(status2, h + 6 * n8 + (size_t)T * 4, (size_t)T * 4);
    if (ran_phase2) memcpy(ran_phase2, h + 7 * n8, (size_t)T);
    return 0;
}

// ---- suggest(SDR) for problems of the unit-diagonal family that share the context's constraints x_i^2 == d_i: the relaxation (mixing
// method), its multipliers and S samples per problem.  ds == nullptr: the context's d; else [B][n], per_problem set (the _pc symbol).
// maxn: SDR_SMALL_MAXN, or SDR_WIDE_MAXN for qcqpmi_sdr_batch[_pc], whose problems of more than SDR_SMALL_MAXN variables run the wide kernel
int sdr_small_batch(qcqpmi_ctx *c, int64_t maxn, bool per_problem, const double *ds, int64_t B, const double *P0s, const double *q0s, const double *r0s,
                    int64_t S, int max_sweeps, double tol, uint64_t seed, uint64_t seed_stride, uint64_t first_index, const double *V0s,
                    double *V, double *primal, double *y, int64_t *sweeps, double *X) {
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
    Carve cv;
    const size_t oP = cv.take((size_t)B * n * n * 8), oq = cv.take((size_t)B * n * 8), or0 = cv.take((size_t)B * 8), os = cv.take((size_t)ns * 8);
    const size_t oV0 = cv.take(V0s ? vbytes : 0), oV = cv.take(vbytes);
    const size_t opr = cv.take((size_t)B * 8), oy = cv.take((size_t)B * N * 8), osw = cv.take((size_t)B * 8), oX = cv.take((size_t)B * S * n * 8);
    const size_t oticket = cv.take(2 * sizeof(int));
    HIPCHK(c, c->ss_work.reserve(c->stream, cv.off, false));
    char *w = c->ss_work;
    std::vector<double> sv((size_t)ns);
    for (int64_t i = 0; i < ns; i++) sv[(size_t)i] = sqrt(ds ? ds[i] : c->unit_d[(size_t)i]);
    if ((rc = stage_in(c, w + oP, P0s, (size_t)B * n * n * 8)) || (rc = stage_in(c, w + oq, q0s, (size_t)B * n * 8)) ||
        (rc = stage_in(c, w + or0, r0s, (size_t)B * 8)) || (rc = stage_in(c, w + os, sv.data(), (size_t)ns * 8)) ||
        (rc = stage_in(c, w + oV0, V0s, vbytes)))
        return rc;
    HIPCHK(c, hipMemsetAsync(w + oticket, 0, 2 * sizeof(int), c->stream));
    HIPCHK(c, spin_sync(c->stream));      // sv goes out of scope; the pageable copies above have been staged
    SdrSmallArgs a;
    a.n = (int)n; a.B = B; a.S = S;
    a.s = (const double *)(w + os); a.s_stride = ds ? n : 0; a.P0s = (const double *)(w + oP); a.q0s = (const double *)(w + oq); a.r0s = (const double *)(w + or0);
    a.V0s = V0s ? (const double *)(w + oV0) : nullptr;
    a.max_sweeps = max_sweeps; a.tol = tol; a.seed = seed; a.seed_stride = seed_stride; a.first_index = first_index;
    a.ticket = (int *)(w + oticket);
    a.V = (double *)(w + oV); a.primal = (double *)(w + opr); a.y = (double *)(w + oy); a.sweeps = (int64_t *)(w + osw); a.X = (double *)(w + oX);
    const int wgs = sdr_small_workgroups((int)n, B, c->device);
    if (wgs < 1) return fail(c, QCQPMI_EHIP, "sdr_small_batch: occupancy query failed: %s", hipGetErrorString((hipError_t)(-wgs)));
    const hipError_t qe = (hipError_t)sdr_small_launch(a, wgs, c->stream);
    if (qe != hipSuccess) return fail(c, QCQPMI_EHIP, "sdr_small_batch: %s", hipGetErrorString(qe));
    if ((rc = check_symmetric(c, w + oticket, "sdr_small_batch: an objective matrix P0_b is not symmetric (or holds a NaN)"))) return rc;
    if (V) HIPCHK(c, hipMemcpyAsync(V, a.V, vbytes, hipMemcpyDeviceToHost, c->stream));
    if (primal) HIPCHK(c, hipMemcpyAsync(primal, a.primal, (size_t)B * 8, hipMemcpyDeviceToHost, c->stream));
    if (y) HIPCHK(c, hipMemcpyAsync(y, a.y, (size_t)B * N * 8, hipMemcpyDeviceToHost, c->stream));
    if (sweeps) HIPCHK(c, hipMemcpyAsync(sweeps, a.sweeps, (size_t)B * 8, hipMemcpyDeviceToHost, c->stream));
    if (X && S > 0) HIPCHK(c, hipMemcpyAsync(X, a.X, (size_t)B * S * n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

// ---- suggest(SPECTRAL) for problems whose constraints aggregate to ONE sphere (relop_eq) or ONE ball: agg = [a (n) | beta (n) | gamma]
// per problem (agg_stride = 2 n + 1) or shared (agg_stride = 0).  The context gives n, the device and the buffer; its constraints are not read.
// maxn: SPECTRAL_SMALL_MAXN, or SPECTRAL_WIDE_MAXN for qcqpmi_spectral_batch, whose problems of more than SPECTRAL_SMALL_MAXN variables run the wide kernel
int spectral_small_batch(qcqpmi_ctx *c, int64_t maxn, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *agg, int64_t agg_stride,
                         int relop_eq, int max_sweeps, double tol, double *x, double *bound, double *mu, double *lam, int64_t *sweeps,
                         int *branch, int *status) {
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
    Carve cv;
    const size_t oP = cv.take((size_t)B * n * n * 8), oq = cv.take((size_t)B * n * 8), or0 = cv.take((size_t)B * 8), oa = cv.take((size_t)nagg * na * 8);
    const size_t ox = cv.take((size_t)B * n * 8), olam = cv.take((size_t)B * n * 8), obd = cv.take((size_t)B * 8), omu = cv.take((size_t)B * 8);
    const size_t osw = cv.take((size_t)B * 8), obr = cv.take((size_t)B * 4), ost = cv.take((size_t)B * 4);
    const size_t oticket = cv.take(2 * sizeof(int));
    HIPCHK(c, c->ss_work.reserve(c->stream, cv.off, false));
    char *w = c->ss_work;
    if ((rc = stage_in(c, w + oP, P0s, (size_t)B * n * n * 8)) || (rc = stage_in(c, w + oq, q0s, (size_t)B * n * 8)) ||
        (rc = stage_in(c, w + or0, r0s, (size_t)B * 8)) || (rc = stage_in(c, w + oa, agg, (size_t)nagg * na * 8)))
        return rc;
    HIPCHK(c, hipMemsetAsync(w + oticket, 0, 2 * sizeof(int), c->stream));
    SpectralSmallArgs a;
    a.n = (int)n; a.B = B;
    a.P0s = (const double *)(w + oP); a.q0s = (const double *)(w + oq); a.r0s = (const double *)(w + or0);
    a.agg = (const double *)(w + oa); a.agg_stride = agg_stride;
    a.relop_eq = relop_eq ? 1 : 0; a.max_sweeps = max_sweeps; a.tol = tol;
    a.ticket = (int *)(w + oticket);
    a.x = (double *)(w + ox); a.bound = (double *)(w + obd); a.mu = (double *)(w + omu); a.lam = (double *)(w + olam);
    a.sweeps = (int64_t *)(w + osw); a.branch = (int *)(w + obr); a.status = (int *)(w + ost);
    const bool wide = n > SPECTRAL_SMALL_MAXN;
    const int wgs = wide ? spectral_wide_workgroups((int)n, B, c->device) : spectral_small_workgroups((int)n, B, c->device);
    if (wgs < 1) return fail(c, QCQPMI_EHIP, "spectral_small_batch: occupancy query failed: %s", hipGetErrorString((hipError_t)(-wgs)));
    const hipError_t qe = (hipError_t)(wide ? spectral_wide_launch(a, wgs, c->stream) : spectral_small_launch(a, wgs, c->stream));
    if (qe != hipSuccess) return fail(c, QCQPMI_EHIP, "spectral_small_batch: %s", hipGetErrorString(qe));
    if ((rc = check_symmetric(c, w + oticket, "spectral_small_batch: an objective matrix P0_b is not symmetric (or holds a NaN)"))) return rc;
    if (x) HIPCHK(c, hipMemcpyAsync(x, a.x, (size_t)B * n * 8, hipMemcpyDeviceToHost, c->stream));
    if (bound) HIPCHK(c, hipMemcpyAsync(bound, a.bound, (size_t)B * 8, hipMemcpyDeviceToHost, c->stream));
    if (mu) HIPCHK(c, hipMemcpyAsync(mu, a.mu, (size_t)B * 8, hipMemcpyDeviceToHost, c->stream));
    if (lam) HIPCHK(c, hipMemcpyAsync(lam, a.lam, (size_t)B * n * 8, hipMemcpyDeviceToHost, c->stream));
    if (sweeps) HIPCHK(c, hipMemcpyAsync(sweeps, a.sweeps, (size_t)B * 8, hipMemcpyDeviceToHost, c->stream));
    if (branch) HIPCHK(c, hipMemcpyAsync(branch, a.branch, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
    if (status) HIPCHK(c, hipMemcpyAsync(status, a.status, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return 0;
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
    for (int64_t b = 0; b < B; b++)
        if (!(rhos[b] > 0.0) || !std::isfinite(rhos[b]))
            return fail(c, QCQPMI_EINVAL, "admm_small_batch_run: rho of problem %lld is not positive and finite", (long long)b);
    if (cons && (rc = check_batch_cons(c, name, cons, B, m))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->n, T = B * R;
    Carve cv;
    const size_t oP = cv.take((size_t)B * n * n * 8), oM = cv.take((size_t)B * n * n * 8), oq = cv.take((size_t)B * n * 8), or0 = cv.take((size_t)B * 8);
    const size_t orho = cv.take((size_t)B * 8);
    const size_t oX0 = cv.take(generate ? 0 : (size_t)T * n * 8), oX = cv.take((size_t)T * n * 8);
    const size_t oout = cv.take((size_t)T * 32);      // 2 x int64, 2 x double per restart, array after array
    const size_t oticket = cv.take(2 * sizeof(int));
    const BatchBest best = {cv.take((size_t)B * 2 * sizeof(int64_t)), cv.take((size_t)B * 2 * sizeof(double)), cv.take((size_t)B * n * 8),
                            best_index, best_f0, best_maxviol, best_x};
    const size_t ocons = cv.take(cons ? (size_t)B * m * 24 : 0);
    HIPCHK(c, c->sb_work.reserve(c->stream, cv.off, false));
    char *w = c->sb_work;
    if ((rc = stage_in(c, w + oP, P0s, (size_t)B * n * n * 8)) || (rc = stage_in(c, w + oM, Minvs, (size_t)B * n * n * 8)) ||
        (rc = stage_in(c, w + oq, q0s, (size_t)B * n * 8)) || (rc = stage_in(c, w + or0, r0s, (size_t)B * 8)) ||
        (rc = stage_in(c, w + orho, rhos, (size_t)B * 8)) || (rc = stage_in(c, w + oX0, generate ? nullptr : X0, (size_t)T * n * 8)) ||
        (rc = stage_in(c, w + ocons, cons, (size_t)B * m * 24)))
        return rc;
    HIPCHK(c, hipMemsetAsync(w + oticket, 0, 2 * sizeof(int), c->stream));
    AdmmSmallArgs a;
    a.P = c->dp; a.B = B; a.R = R;
    a.P0s = (const double *)(w + oP); a.Minvs = (const double *)(w + oM); a.q0s = (const double *)(w + oq); a.r0s = (const double *)(w + or0);
    a.rhos = (const double *)(w + orho);
    a.X0 = generate ? nullptr : (const double *)(w + oX0);
    a.cons = cons ? (const double *)(w + ocons) : nullptr;
    a.generate = generate ? 1 : 0; a.phase1 = phase1 ? 1 : 0; a.num_iters = num_iters; a.tol = tol; a.viol_lim = viol_lim;
    a.seed = seed; a.seed_stride = seed_stride; a.first_index = first_index;
    a.ticket = (int *)(w + oticket);
    char *o = w + oout;
    a.iters1 = (int64_t *)o; a.iters2 = (int64_t *)(o + 8 * T); a.f0 = (double *)(o + 16 * T); a.maxviol = (double *)(o + 24 * T);
    a.X = (double *)(w + oX);
    const int maxc = c->maxc <= 1 ? 1 : 4;
    int threads = 0;
    const int cap = admm_small_workgroups(n, maxc, cons ? m : 0, B * R, c->device, &threads);
    if (cap < 1) return fail(c, QCQPMI_EHIP, "admm_small_batch_run: occupancy query failed: %s", hipGetErrorString((hipError_t)(-cap)));
    const TicketPlan plan = ticket_partition(B, R, cap, threads / 64);      // workgroups of four waves; four or eight in the wide kernels
    a.RC = plan.RC; a.chunks = plan.chunks;
    const hipError_t qe = (hipError_t)admm_small_launch(a, maxc, plan.wgs, threads, c->stream);
    if (qe != hipSuccess) return fail(c, QCQPMI_EHIP, "admm_small_batch_run: %s", hipGetErrorString(qe));
    c->last_admm_kernel = admm_small_name(maxc, cons != nullptr, n > ADMM_SMALL_MAXN);
    c->last_admm_C = 0;
    if ((rc = select_batch_best(c, name, w, best, a.f0, a.maxviol, a.X, B, R, n, select_tol))) return rc;
    std::vector<char> hout((size_t)T * 32);      // (megabytes of fresh pages: touched while the kernel runs)
    if ((rc = check_symmetric(c, w + oticket, "admm_small_batch_run: a matrix P0_b or Minv_b is not symmetric (or holds a NaN)"))) return rc;
    HIPCHK(c, hipMemcpyAsync(hout.data(), o, hout.size(), hipMemcpyDeviceToHost, c->stream));
    if (X) HIPCHK(c, hipMemcpyAsync(X, a.X, (size_t)T * n * 8, hipMemcpyDeviceToHost, c->stream));
    if ((rc = fetch_batch_best(c, w, best, B, n))) return rc;
    const size_t n8 = (size_t)T * 8;
    void *const outs[4] = {iters1, iters2, f0, maxviol};
    for (size_t k = 0; k < 4; k++) if (outs[k]) memcpy(outs[k], hout.data() + k * n8, n8);
    return 0;
}

// ---- improve([method, ...]): up to CHAIN_MAX_STAGES stages of CD or ADMM one after the other in ONE launch (chain_small.h).  The
// per-stage records live in one block of the work buffer, array after array, every array [nstages][B R] and zeroed before the launch:
// six of int64 (sweeps1, sweeps2, visits2, accepted2, iters1, iters2), two of double (f0, maxviol), two of int (status1, status2), one
// of uint8 (ran_phase2): 73 bytes per stage and restart.  The final f0 / maxviol are the last stage's rows of the two double arrays.
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
        for (int64_t b = 0; b < B; b++)
            if (!(rhos[b] > 0.0) || !std::isfinite(rhos[b]))
                return fail(c, QCQPMI_EINVAL, "chain_small_batch_run: rho of problem %lld is not positive and finite", (long long)b);
    }
    if (cons && (rc = check_batch_cons(c, name, cons, B, m))) return rc;
    if (m == 0) cons = nullptr;       // nothing to stage: the shared kernels
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->n, T = B * R, ST = (int64_t)nstages * T;
    Carve cv;
    const size_t oP = cv.take((size_t)B * n * n * 8), oM = cv.take(any_admm ? (size_t)B * n * n * 8 : 0), oq = cv.take((size_t)B * n * 8), or0 = cv.take((size_t)B * 8);
    const size_t orho = cv.take(any_admm ? (size_t)B * 8 : 0);
    const size_t oX0 = cv.take(generate ? 0 : (size_t)T * n * 8), oX = cv.take((size_t)T * n * 8);
    const size_t oout = cv.take((size_t)ST * 73);
    const size_t oticket = cv.take(2 * sizeof(int));
    const BatchBest best = {cv.take((size_t)B * 2 * sizeof(int64_t)), cv.take((size_t)B * 2 * sizeof(double)), cv.take((size_t)B * n * 8),
                            best_index, best_f0, best_maxviol, best_x};
    const size_t ocons = cv.take(cons ? (size_t)B * m * 24 : 0);
    HIPCHK(c, c->sb_work.reserve(c->stream, cv.off, false));
    char *w = c->sb_work;
    if ((rc = stage_in(c, w + oP, P0s, (size_t)B * n * n * 8)) || (rc = stage_in(c, w + oM, any_admm ? Minvs : nullptr, (size_t)B * n * n * 8)) ||
        (rc = stage_in(c, w + oq, q0s, (size_t)B * n * 8)) || (rc = stage_in(c, w + or0, r0s, (size_t)B * 8)) ||
        (rc = stage_in(c, w + orho, any_admm ? rhos : nullptr, (size_t)B * 8)) || (rc = stage_in(c, w + oX0, generate ? nullptr : X0, (size_t)T * n * 8)) ||
        (rc = stage_in(c, w + ocons, cons, (size_t)B * m * 24)))
        return rc;
    HIPCHK(c, hipMemsetAsync(w + oticket, 0, 2 * sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(w + oout, 0, (size_t)ST * 73, c->stream));      // what a stage does not produce stays zero
    ChainSmallArgs a;
    a.P = c->dp; a.B = B; a.R = R;
    a.P0s = (const double *)(w + oP); a.q0s = (const double *)(w + oq); a.r0s = (const double *)(w + or0);
    a.rhos = any_admm ? (const double *)(w + orho) : nullptr; a.Minvs = any_admm ? (const double *)(w + oM) : nullptr;
    a.X0 = generate ? nullptr : (const double *)(w + oX0);
    a.cons = cons ? (const double *)(w + ocons) : nullptr;
    a.generate = generate ? 1 : 0; a.nstages = nstages;
    a.seed = seed; a.seed_stride = seed_stride; a.first_index = first_index;
    a.ticket = (int *)(w + oticket);
    a.X = (double *)(w + oX);
    char *o = w + oout;
    const size_t a8 = (size_t)ST * 8;      // one array of 8-byte entries
    for (int s = 0; s < CHAIN_MAX_STAGES; s++) {
        ChainStage &g = a.st[s];
        memset(&g, 0, sizeof(g));
        if (s >= nstages) continue;
        g.method = stages[s].method; g.phase1 = stages[s].phase1 ? 1 : 0; g.num_iters = stages[s].num_iters;
        g.tol = stages[s].tol; g.viol_tol = stages[s].viol_tol; g.viol_lim = stages[s].viol_lim;
        const size_t r8 = (size_t)s * T * 8;
        g.sweeps1 = (int64_t *)(o + r8); g.sweeps2 = (int64_t *)(o + a8 + r8); g.visits2 = (int64_t *)(o + 2 * a8 + r8);
        g.accepted2 = (int64_t *)(o + 3 * a8 + r8); g.iters1 = (int64_t *)(o + 4 * a8 + r8); g.iters2 = (int64_t *)(o + 5 * a8 + r8);
        g.f0 = (double *)(o + 6 * a8 + r8); g.maxviol = (double *)(o + 7 * a8 + r8);
        g.status1 = (int *)(o + 8 * a8 + r8 / 2); g.status2 = (int *)(o + 8 * a8 + a8 / 2 + r8 / 2);
        g.ran2 = (uint8_t *)(o + 9 * a8 + r8 / 8);
    }
    const int maxc = c->maxc <= 1 ? 1 : 4;
    const int cap = chain_small_workgroups(n, maxc, cons ? m : 0, B * R, c->device);
    if (cap < 1) return fail(c, QCQPMI_EHIP, "chain_small_batch_run: occupancy query failed: %s", hipGetErrorString((hipError_t)(-cap)));
    const TicketPlan plan = ticket_partition(B, R, cap, 4);      // workgroups of four waves
    a.RC = plan.RC; a.chunks = plan.chunks;
    (void)hipEventRecord(c->timers[2].beg, c->stream);
    const hipError_t qe = (hipError_t)chain_small_launch(a, maxc, plan.wgs, c->stream);
    (void)hipEventRecord(c->timers[2].end, c->stream);
    c->timers[2].valid = true;
    if (qe != hipSuccess) return fail(c, QCQPMI_EHIP, "chain_small_batch_run: %s", hipGetErrorString(qe));
    c->last_cd2_kernel = chain_small_name(maxc, cons != nullptr);
    const ChainStage &last = a.st[nstages - 1];
    if ((rc = select_batch_best(c, name, w, best, last.f0, last.maxviol, a.X, B, R, n, select_tol))) return rc;
    std::vector<char> hout((size_t)ST * 73);      // (megabytes of fresh pages: touched while the kernel runs)
    if ((rc = check_symmetric(c, w + oticket, "chain_small_batch_run: a matrix P0_b or Minv_b is not symmetric (or holds a NaN)"))) return rc;
    HIPCHK(c, hipMemcpyAsync(hout.data(), o, hout.size(), hipMemcpyDeviceToHost, c->stream));
    if (X) HIPCHK(c, hipMemcpyAsync(X, a.X, (size_t)T * n * 8, hipMemcpyDeviceToHost, c->stream));
    if ((rc = fetch_batch_best(c, w, best, B, n))) return rc;
    const char *h = hout.data();
    void *const wide[8] = {st_sweeps1, st_sweeps2, st_visits2, st_accepted2, st_iters1, st_iters2, st_f0, st_maxviol};
    for (size_t k = 0; k < 8; k++) if (wide[k]) memcpy(wide[k], h + k * a8, a8);
    if (st_status1) memcpy(st_status1, h + 8 * a8, a8 / 2);
    if (st_status2) memcpy(st_status2, h + 8 * a8 + a8 / 2, a8 / 2);
    if (st_ran_phase2) memcpy(st_ran_phase2, h + 9 * a8, (size_t)ST);
    const size_t l8 = (size_t)(nstages - 1) * T * 8;
    if (f0) memcpy(f0, h + 6 * a8 + l8, (size_t)T * 8);
    if (maxviol) memcpy(maxviol, h + 7 * a8 + l8, (size_t)T * 8);
    return 0;
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
    Carve cv;
    const size_t oP = cv.take((size_t)B * n * n * 8), oM = cv.take((size_t)B * n * n * 8), orho = cv.take((size_t)B * 8), olm = cv.take((size_t)B * 8);
    const size_t osw = cv.take((size_t)B * 8), ost = cv.take((size_t)B * 4), oticket = cv.take(2 * sizeof(int));
    HIPCHK(c, c->ss_work.reserve(c->stream, cv.off, false));
    char *w = c->ss_work;
    if ((rc = stage_in(c, w + oP, P0s, (size_t)B * n * n * 8))) return rc;
    HIPCHK(c, hipMemsetAsync(w + oticket, 0, 2 * sizeof(int), c->stream));
    if (rho) HIPCHK(c, hipMemsetAsync(w + oM, 0, (size_t)B * n * n * 8, c->stream));      // a problem of status 3 is not written
    AdmmSetupArgs a;
    a.n = (int)n; a.B = B;
    a.P0s = (const double *)(w + oP);
    a.m = (double)m; a.has_rho = rho ? 1 : 0; a.rho = rho ? *rho : 0.0;
    a.max_sweeps = max_sweeps; a.tol = tol;
    a.ticket = (int *)(w + oticket);
    a.rhos = (double *)(w + orho); a.lambda_min = (double *)(w + olm); a.Minvs = (double *)(w + oM);
    a.sweeps = (int64_t *)(w + osw); a.status = (int *)(w + ost);
    const int wgs = admm_setup_workgroups((int)n, B, c->device);
    if (wgs < 1) return fail(c, QCQPMI_EHIP, "admm_batch_setup: occupancy query failed: %s", hipGetErrorString((hipError_t)(-wgs)));
    const hipError_t qe = (hipError_t)admm_setup_launch(a, wgs, c->stream);
    if (qe != hipSuccess) return fail(c, QCQPMI_EHIP, "admm_batch_setup: %s", hipGetErrorString(qe));
    if ((rc = check_symmetric(c, w + oticket, "admm_batch_setup: an objective matrix P0_b is not symmetric (or holds a NaN)"))) return rc;
    if (rhos) HIPCHK(c, hipMemcpyAsync(rhos, a.rhos, (size_t)B * 8, hipMemcpyDeviceToHost, c->stream));
    if (lambda_min) HIPCHK(c, hipMemcpyAsync(lambda_min, a.lambda_min, (size_t)B * 8, hipMemcpyDeviceToHost, c->stream));
    if (Minvs) HIPCHK(c, hipMemcpyAsync(Minvs, a.Minvs, (size_t)B * n * n * 8, hipMemcpyDeviceToHost, c->stream));
    if (sweeps) HIPCHK(c, hipMemcpyAsync(sweeps, a.sweeps, (size_t)B * 8, hipMemcpyDeviceToHost, c->stream));
    if (status) HIPCHK(c, hipMemcpyAsync(status, a.status, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return 0;
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
