// C ABI of libqcqp_mi.so (declared in include/qcqp_mi.h): context and error slot, problem upload and finalize, population
// management, evaluation, SDR sampling and the mixing-method solver, selection, HIP-event timing; launches of the kernels in
// kernels_impl.h and sdr_solve.h.  The core of the host side: coordinate descent on the resident population is in capi_cd.hip, the
// dense-constraint path in capi_dense.hip, the ADMM calls in capi_admm.hip, the small-problem batch calls in capi_small.hip, the
// unit operators in capi_units.hip, RCCL in capi_comm.hip, the streamed coordinate descent (qcqpmi_cd_stream_run and what it
// needs: host code only) in capi_stream.hip; capi_ctx.h holds what these units share.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "capi_ctx.h"
#include "kernels_impl.h"
#include "sdr_solve.h"

using namespace qcqpmi;

namespace {

thread_local std::string g_create_error;      // the ONE slot of errors without a context: fail() writes it, qcqpmi_last_error(NULL) reads it

}  // namespace

namespace qcqpmi {

int fail(qcqpmi_ctx *c, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

int check_ready(qcqpmi_ctx *c, bool need_pop) {
    if (!c) return QCQPMI_EINVAL;
    if (!c->finalized) return fail(c, QCQPMI_ESTATE, "qcqpmi_finalize has not been called");
    if (need_pop && c->R <= 0) return fail(c, QCQPMI_ESTATE, "no resident population (upload / randn / sdr_sample first)");
    return 0;
}

void launch_select_best(qcqpmi_ctx *c, int64_t pops, const double *f0, const double *maxviol, int64_t R, double tol, int64_t *out_idx,
                        double *out_key) {
    hipLaunchKernelGGL(select_best_kernel, dim3((unsigned)pops), dim3(1024), 0, c->stream, f0, maxviol, R, tol, out_idx, out_key);
}

void launch_from_tiles(qcqpmi_ctx *c, const double *Xt, int64_t R) {
    const int64_t total = R * c->n;
    hipLaunchKernelGGL(from_tiles_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, Xt, c->d_stage, c->n, c->n16, R);
}

}  // namespace qcqpmi

namespace {

void free_population(qcqpmi_ctx *c) {
    c->X.release(); c->Xi.release(); c->d_f0.release(); c->d_mv.release(); c->d_F.release(); c->d_stage.release();
    c->d_visits.release(); c->d_acc.release(); c->d_sweeps.release(); c->d_sweeps1.release();
    c->d_status.release(); c->d_status1.release(); c->d_flag.release();
    c->Rcap = 0;
}

}  // namespace

namespace qcqpmi {

int pop_reserve(qcqpmi_ctx *c, int64_t R) {
    if (R <= 0) return fail(c, QCQPMI_EINVAL, "population size must be positive");
    int64_t Rpad = (R + 15) / 16 * 16;
    if (Rpad > c->Rcap) {
        HIPCHK(c, spin_sync(c->stream));
        free_population(c);
        const size_t Rp = (size_t)Rpad;
        HIPCHK(c, c->X.reserve(c->stream, Rp * (size_t)c->n16));
        HIPCHK(c, c->d_stage.reserve(c->stream, Rp * (size_t)c->n));
        HIPCHK(c, c->d_f0.reserve(c->stream, Rp));
        HIPCHK(c, c->d_mv.reserve(c->stream, Rp));
        HIPCHK(c, c->d_visits.reserve(c->stream, Rp));
        HIPCHK(c, c->d_acc.reserve(c->stream, Rp));
        HIPCHK(c, c->d_sweeps.reserve(c->stream, Rp));
        HIPCHK(c, c->d_sweeps1.reserve(c->stream, Rp));
        HIPCHK(c, c->d_status.reserve(c->stream, Rp));
        HIPCHK(c, c->d_status1.reserve(c->stream, Rp));
        HIPCHK(c, c->d_flag.reserve(c->stream, Rp));
        c->Rcap = Rpad;
    }
    c->R = R;
    c->Rpad = Rpad;
    c->evaluated = false;
    return 0;
}

void launch_gather_best_x(qcqpmi_ctx *c, int64_t pops, int64_t R, const int64_t *idx, double *out) {
    hipLaunchKernelGGL(gather_best_x_kernel, dim3((unsigned)pops), dim3(256), 0, c->stream, (const double *)c->X, c->n, c->n16, R, idx, out);
}

int launch_eval(qcqpmi_ctx *c, bool want_F) {
    if (dense_on(c)) return launch_eval_dense(c, false);   // coupled constraints: every function on the matrix cores
    if (want_F) HIPCHK(c, c->d_F.reserve(c->stream, (size_t)((c->m + 1) * c->Rpad)));
    EvalArgs a;
    a.P = c->dp; a.X = c->X; a.R = c->R; a.f0 = c->d_f0; a.maxviol = c->d_mv;
    a.F = want_F ? c->d_F : nullptr; a.Rpad = c->Rpad;
    a.planes = nullptr; a.nplanes = 0;
    tic(c, 0);
    const int NB = (int)(c->n16 / 16), ntiles = (int)(c->Rpad / 16);
    if (NB >= 8 && ntiles >= 8) {
        // x'P0x through the LDS-tiled GEMM of the dense unit, in partial planes that eval_kernel sums
        const int nplanes = dense_product_planes(NB);
        HIPCHK(c, c->d_planes.reserve(c->stream, (size_t)nplanes * c->Rpad));
        int rc = launch_dense_product(c, 2, c->dp.Apack, nullptr, c->X, c->d_planes);
        if (rc) return rc;
        a.planes = c->d_planes; a.nplanes = nplanes;
    }
    hipLaunchKernelGGL(eval_kernel, dim3((unsigned)(c->Rpad / 16)), dim3(256), 0, c->stream, a);
    toc(c, 0);
    HIPCHK(c, hipGetLastError());
    c->evaluated = true;
    return 0;
}

}  // namespace qcqpmi

// ============================================================================================

extern "C" {

int qcqpmi_abi_version(void) { return QCQPMI_ABI_VERSION; }

int qcqpmi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *qcqpmi_last_error(const qcqpmi_ctx *ctx) {
    return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

int qcqpmi_ctx_create(qcqpmi_ctx **out, int64_t n, int64_t m, int device) {
    if (!out || n <= 0 || m < 0) return fail(nullptr, QCQPMI_EINVAL, "ctx_create: bad arguments");
    int ndev = qcqpmi_device_count();
    if (ndev <= 0)
        return fail(nullptr, QCQPMI_EHIP, "no HIP device visible: the qcqp_amd engine requires an MI355X (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, QCQPMI_EINVAL, "device %d out of range (%d visible)", device, ndev);
    qcqpmi_ctx *c = new qcqpmi_ctx();
    c->device = device; c->n = n; c->m = m; c->n16 = (n + 15) / 16 * 16;
    c->quads.resize((size_t)m + 1);
    if (const char *sl = getenv("QCQPMI_STREAM_LIMIT")) { const double v = atof(sl); if (v > 0.0) c->stream_limit = v; }   // tests: exercise the streaming upload at small sizes
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int i = 0; i < 5 && e == hipSuccess; i++) {
        e = hipEventCreate(&c->timers[i].beg);
        if (e == hipSuccess) e = hipEventCreate(&c->timers[i].end);
    }
    if (e != hipSuccess) {
        int rc = fail(nullptr, QCQPMI_EHIP, "ctx_create: %s", hipGetErrorString(e));
        delete c;
        return rc;
    }
    *out = c;
    return 0;
}

void qcqpmi_ctx_destroy(qcqpmi_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)spin_sync(c->stream);
    comm_drop(c);
    admm_drop_handle(c);
    for (auto &t : c->timers) { if (t.beg) (void)hipEventDestroy(t.beg); if (t.end) (void)hipEventDestroy(t.end); }
    for (auto &e : c->dn_ev) if (e) (void)hipEventDestroy(e);
    for (auto &e : c->dn_evn) if (e) (void)hipEventDestroy(e);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;      // every buffer frees itself (the stream was idle above: nothing in flight reads one)
}

int qcqpmi_set_quad(qcqpmi_ctx *c, int64_t k, int format, const double *vals, const int64_t *idx,
                    const int64_t *ptr, int64_t nnz, const double *q, double r, int relop) {
    if (!c) return QCQPMI_EINVAL;
    if (c->finalized) return fail(c, QCQPMI_ESTATE, "set_quad after finalize");
    if (k < 0 || k > c->m || !q) return fail(c, QCQPMI_EINVAL, "set_quad: bad k or q");
    if ((k == 0) != (relop == 0) || relop < 0 || relop > 2)
        return fail(c, QCQPMI_EINVAL, "set_quad: relop %d invalid for function %lld", relop, (long long)k);
    HostQuad &h = c->quads[(size_t)k];
    h = HostQuad();
    const int64_t n = c->n;
    if (format == QCQPMI_FMT_DENSE) {
        if (!vals) return fail(c, QCQPMI_EINVAL, "set_quad: dense vals missing");
        for (int64_t i = 0; i < n; i++)
            for (int64_t j = 0; j < n; j++) {
                double v = vals[i * n + j];
                if (v != 0.0) { h.ci.push_back((int)i); h.cj.push_back((int)j); h.cv.push_back(v); }
            }
    } else if (format == QCQPMI_FMT_CSR) {
        if (!ptr || (nnz > 0 && (!idx || !vals))) return fail(c, QCQPMI_EINVAL, "set_quad: CSR arrays missing");
        for (int64_t i = 0; i < n; i++)
            for (int64_t e = ptr[i]; e < ptr[i + 1]; e++) {
                if (idx[e] < 0 || idx[e] >= n || e >= nnz) return fail(c, QCQPMI_EINVAL, "set_quad: CSR index out of range");
                if (vals[e] != 0.0) { h.ci.push_back((int)i); h.cj.push_back((int)idx[e]); h.cv.push_back(vals[e]); }
            }
    } else {
        return fail(c, QCQPMI_EINVAL, "set_quad: unknown format %d", format);
    }
    // P must be symmetric (include/qcqp_mi.h): get_onevar_func (utilities.py:99-105) and the in-block
    // Gauss-Seidel fold read P[k, j] where the mathematics has P[j, k].  The reference symmetrises in
    // get_qcqp_form (utilities.py:333, 345); raw arrays are checked here instead of being trusted.
    if (format == QCQPMI_FMT_DENSE) {
        for (int64_t i = 0; i < n; i++)
            for (int64_t j = i + 1; j < n; j++)
                if (vals[i * n + j] != vals[j * n + i])
                    return fail(c, QCQPMI_EINVAL, "set_quad: P of function %lld is not symmetric (entry %lld,%lld); pass (P + P^T)/2",
                                (long long)k, (long long)i, (long long)j);
    } else {
        std::vector<std::pair<int64_t, double>> ent(h.cv.size());
        for (size_t e = 0; e < h.cv.size(); e++) ent[e] = {(int64_t)h.ci[e] * n + h.cj[e], h.cv[e]};
        std::sort(ent.begin(), ent.end(), [](const std::pair<int64_t, double> &a, const std::pair<int64_t, double> &b) { return a.first < b.first; });
        size_t w = 0;
        for (size_t e = 0; e < ent.size(); e++) {   // duplicates add up (COO semantics)
            if (w > 0 && ent[w - 1].first == ent[e].first) ent[w - 1].second += ent[e].second;
            else ent[w++] = ent[e];
        }
        ent.resize(w);
        for (const auto &en : ent) {
            const int64_t i = en.first / n, j = en.first % n;
            if (i == j) continue;
            const int64_t tk = j * n + i;
            auto it = std::lower_bound(ent.begin(), ent.end(), tk, [](const std::pair<int64_t, double> &a, int64_t key) { return a.first < key; });
            const double tv = (it != ent.end() && it->first == tk) ? it->second : 0.0;
            if (tv != en.second)
                return fail(c, QCQPMI_EINVAL, "set_quad: P of function %lld is not symmetric (entry %lld,%lld); pass (P + P^T)/2",
                            (long long)k, (long long)i, (long long)j);
        }
    }
    bool coupled = false;      // does the function touch more than one coordinate?  (separable constraints stay per-coordinate lists)
    {
        int64_t coord = -1;
        for (size_t e = 0; e < h.cv.size() && !coupled; e++) {
            if (h.ci[e] != h.cj[e] || (coord >= 0 && coord != h.ci[e])) coupled = true;
            coord = h.ci[e];
        }
        for (int64_t j = 0; j < n && !coupled; j++)
            if (q[j] != 0.0) { if (coord >= 0 && coord != j) coupled = true; coord = j; }
    }
    if (k >= 1 && coupled && (double)c->m * (double)n * (double)n * 8.0 > c->stream_limit) {
        // ---- streaming upload: the row-major copy of all constraint matrices would not fit the budget (16 GB; BASELINE.json
        // configs[4] is 137 GB).  The function goes to the device now, straight into the block-major fragment layout of the
        // dense path (cd_dense.h); its entries are not kept on the host.  Such a problem runs on the dense path only.
        const int64_t n16 = c->n16, m1 = c->m + 1;
        if ((double)m1 * (double)n16 * (double)n16 * 8.0 > 200e9)
            return fail(c, QCQPMI_EUNSUPPORTED, "set_quad: %lld matrices of %lld x %lld exceed the 200 GB kept for packed matrices", (long long)m1, (long long)n, (long long)n);
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, c->dn_gp_pre.reserve(c->stream, (size_t)m1 * n16 * n16, false));
        HIPCHK(c, c->dn_tmp.reserve(c->stream, (size_t)n * n, false));
        std::vector<double> dense;
        const double *src = vals;
        if (format != QCQPMI_FMT_DENSE) {
            dense.assign((size_t)n * n, 0.0);
            for (size_t e = 0; e < h.cv.size(); e++) dense[(size_t)h.ci[e] * n + h.cj[e]] += h.cv[e];
            src = dense.data();
        }
        HIPCHK(c, hipMemcpyAsync(c->dn_tmp, src, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        launch_dense_pack_staged(c, k, c->dn_gp_pre);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, spin_sync(c->stream));      // the staging buffer and the caller's array are free again
        std::vector<int>().swap(h.ci); std::vector<int>().swap(h.cj); std::vector<double>().swap(h.cv);
        h.streamed = true;
    }
    h.q.assign(q, q + n);
    h.r = r; h.relop = relop; h.set = true;
    return 0;
}

int qcqpmi_finalize(qcqpmi_ctx *c) {
    if (!c) return QCQPMI_EINVAL;
    if (c->finalized) return 0;
    for (size_t k = 0; k < c->quads.size(); k++)
        if (!c->quads[k].set) return fail(c, QCQPMI_ESTATE, "finalize: function %zu was never set", k);
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->n, n16 = c->n16, m = c->m;
    DevProblem &dp = c->dp;
    dp.n = n; dp.n16 = n16; dp.NB = n16 / 16; dp.KS = n16 / 4; dp.m = m;
    // ---- objective: dense padded + MFMA-packed
    {
        const HostQuad &h = c->quads[0];
        std::vector<double> P((size_t)n16 * n16, 0.0), q((size_t)n16, 0.0);
        for (size_t e = 0; e < h.cv.size(); e++) P[(size_t)h.ci[e] * n16 + h.cj[e]] += h.cv[e];
        for (int64_t j = 0; j < n; j++) q[j] = h.q[j];
        int rc;
        if (h.gen) {   // generated on the device, mirrored to the host for the diagonal classification below
            DevBuf<double> tmp;
            HIPCHK(c, tmp.reserve(c->stream, (size_t)n16 * n16, false));
            launch_dense_gen_rowmajor(c, tmp.p, 0, h.gseed, h.gscale, h.gdiag);
            HIPCHK(c, hipMemcpyAsync(P.data(), tmp.p, P.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, spin_sync(c->stream));
        }
        {
            bool dg = true;
            for (size_t e = 0; e < h.cv.size() && dg; e++) dg = h.ci[e] == h.cj[e];
            c->p0_diag = dg && !h.gen;
            c->p0_diag_host.assign((size_t)n, 0.0);
            for (int64_t i = 0; i < n; i++) c->p0_diag_host[(size_t)i] = P[(size_t)i * n16 + i];
        }
        if ((rc = prob_upload(c, &dp.P0, P))) return rc;
        if ((rc = prob_upload(c, &dp.q0, q))) return rc;
        std::vector<double> rcp2d((size_t)n16, 0.0);
        for (int64_t i = 0; i < n; i++) {
            const double d = P[(size_t)i * n16 + i];
            if (d != 0.0) rcp2d[i] = 1.0 / (2.0 * d);
        }
        if ((rc = prob_upload(c, &dp.rcp2d, rcp2d))) return rc;
        {
            bool allpos = true, allzero = true;
            for (int64_t i = 0; i < n; i++) {
                const double d = P[(size_t)i * n16 + i];
                allpos = allpos && d > 0.0;
                allzero = allzero && d == 0.0;
            }
            c->objclass = allpos ? 1 : (allzero ? 2 : 0);
            double fb = fabs(h.r);
            for (int64_t i = 0; i < n; i++) {
                fb += fabs(q[(size_t)i]);
                for (int64_t j = 0; j < n; j++) fb += fabs(P[(size_t)i * n16 + j]);
            }
            c->fbound = fb;
        }
        double *ap = nullptr;
        if ((rc = prob_alloc(c, &ap, (size_t)n16 * n16))) return rc;
        int64_t total = n16 * n16;
        hipLaunchKernelGGL(pack_A_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream,
                           dp.P0, ap, n16, dp.KS);
        HIPCHK(c, hipGetLastError());
        double *ap2 = nullptr;
        if ((rc = prob_alloc(c, &ap2, (size_t)n16 * n16))) return rc;
        hipLaunchKernelGGL(pack_A2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream,
                           dp.P0, ap2, n16, dp.KS);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, spin_sync(c->stream));  // P, q vectors go out of scope
        dp.Apack = ap;
        dp.Apack2 = ap2;
        dp.r0 = h.r;
    }
    // ---- constraints: separable iff one diagonal entry / one linear entry on the same coordinate
    bool sep = true;
    std::vector<int> coord_of((size_t)m, -1);
    for (int64_t k = 1; k <= m && sep; k++) {
        const HostQuad &h = c->quads[(size_t)k];
        int coord = -1;
        if (h.gen || h.streamed) { sep = false; break; }
        for (size_t e = 0; e < h.cv.size(); e++) {
            if (h.ci[e] != h.cj[e]) { sep = false; break; }
            if (coord >= 0 && coord != h.ci[e]) { sep = false; break; }
            coord = h.ci[e];
        }
        for (int64_t j = 0; j < n && sep; j++)
            if (h.q[j] != 0.0) { if (coord >= 0 && coord != (int)j) sep = false; coord = (int)j; }
        if (coord < 0) sep = false;  // constant constraint
        coord_of[(size_t)k - 1] = coord;
    }
    if (sep) {
        // the per-lane one-variable solver holds at most 4 constraints per coordinate (onevar.h); problems with more go
        // through the paths for general constraints below, which take any number (utilities.py:241-255 takes any m)
        std::vector<int> per((size_t)n, 0);
        for (int64_t k = 0; k < m && sep; k++) sep = ++per[(size_t)coord_of[k]] <= 4;
    }
    c->sep = sep;
    dp.sep = sep ? 1 : 0;
    int rc;
    if (sep) {
        std::vector<int> cptr((size_t)n16 + 1, 0);
        for (int64_t k = 0; k < m; k++) cptr[(size_t)coord_of[k] + 1]++;
        int maxc = 0;
        for (int64_t i = 0; i < n16; i++) { maxc = std::max(maxc, cptr[i + 1]); cptr[i + 1] += cptr[i]; }
        std::vector<double> cp((size_t)m), cq((size_t)m), cr((size_t)m);
        std::vector<int> crel((size_t)m), cidx((size_t)m), fill(cptr.begin(), cptr.end() - 1);
        for (int64_t k = 0; k < m; k++) {  // constraint order preserved inside a coordinate's list
            const HostQuad &h = c->quads[(size_t)k + 1];
            int i = coord_of[k], e = fill[i]++;
            double p = 0.0;
            for (size_t t = 0; t < h.cv.size(); t++) p += h.cv[t];
            cp[e] = p; cq[e] = h.q[i]; cr[e] = h.r; crel[e] = h.relop; cidx[e] = (int)k + 1;
        }
        c->maxc = maxc; dp.maxc = maxc;
        c->unit_d.clear();
        if (m == n) {
            std::vector<double> d((size_t)n, 0.0);
            bool fam = true;
            for (int64_t i = 0; i < n && fam; i++) {
                const int e = cptr[i];
                fam = cptr[i + 1] - e == 1 && cq[e] == 0.0 && crel[e] == RELOP_EQ && cp[e] != 0.0;
                if (fam) { d[(size_t)i] = -cr[e] / cp[e]; fam = d[(size_t)i] > 0.0; }
            }
            if (fam) c->unit_d = d;
        }
        // constraint classes: coordinates whose (p, q, r, relop) lists are bit-identical
        {
            std::vector<int> cls((size_t)n16, 0), krep;
            for (int64_t i = 0; i < n16; i++) {
                int found = -1;
                const int len = cptr[i + 1] - cptr[i];
                for (size_t k = 0; k < krep.size() && found < 0; k++) {
                    const int j = krep[k];
                    if (cptr[j + 1] - cptr[j] != len) continue;
                    bool same = true;
                    for (int e = 0; e < len && same; e++) {
                        const int a = cptr[i] + e, b = cptr[j] + e;
                        same = memcmp(&cp[a], &cp[b], 8) == 0 && memcmp(&cq[a], &cq[b], 8) == 0 &&
                               memcmp(&cr[a], &cr[b], 8) == 0 && crel[a] == crel[b];
                    }
                    if (same) found = (int)k;
                }
                if (found < 0) {
                    krep.push_back((int)i);
                    found = (int)krep.size() - 1;
                }
                cls[i] = found;
            }
            dp.K = (int)krep.size();
            c->K = dp.K;
            {
                std::vector<char> seen(krep.size(), 0);
                int kr = 0;
                for (int64_t i = 0; i < n; i++) if (!seen[(size_t)cls[i]]) { seen[(size_t)cls[i]] = 1; kr++; }
                c->Kreal = kr;
            }
            c->symcls = false;
            if (c->Kreal == 1 && maxc == 1) {        // (Kreal: the padded coordinates of n16 form a class of their own)
                const int e0 = cptr[krep[0]];
                c->symcls = cq[e0] == 0.0 && crel[e0] == RELOP_EQ && cp[e0] != 0.0;
            }
            if ((rc = prob_upload(c, &dp.krep, krep))) return rc;
            if ((rc = prob_upload(c, &dp.cls, cls))) return rc;
        }
        if ((rc = prob_upload(c, &dp.cptr, cptr))) return rc;
        if ((rc = prob_upload(c, &dp.cp, cp))) return rc;
        if ((rc = prob_upload(c, &dp.cq, cq))) return rc;
        if ((rc = prob_upload(c, &dp.cr, cr))) return rc;
        if ((rc = prob_upload(c, &dp.crel, crel))) return rc;
        if ((rc = prob_upload(c, &dp.cidx, cidx))) return rc;
    } else {
        std::vector<int64_t> gptr((size_t)m + 1, 0);
        std::vector<int> gi, gj, grel((size_t)m);
        std::vector<double> gv, gq((size_t)m * n16, 0.0), gr((size_t)m);
        for (int64_t k = 0; k < m; k++) {
            const HostQuad &h = c->quads[(size_t)k + 1];
            gi.insert(gi.end(), h.ci.begin(), h.ci.end());
            gj.insert(gj.end(), h.cj.begin(), h.cj.end());
            gv.insert(gv.end(), h.cv.begin(), h.cv.end());
            gptr[(size_t)k + 1] = (int64_t)gv.size();
            for (int64_t j = 0; j < n; j++) gq[(size_t)k * n16 + j] = h.q[j];
            gr[k] = h.r; grel[k] = h.relop;
        }
        bool all_gen = true;
        for (int64_t k = 1; k <= m; k++) all_gen = all_gen && c->quads[(size_t)k].gen;
        c->dn_force = false;
        bool any_streamed = false;
        for (int64_t k = 0; k <= m; k++) { c->dn_force = c->dn_force || c->quads[(size_t)k].gen || c->quads[(size_t)k].streamed; any_streamed = any_streamed || c->quads[(size_t)k].streamed; }
        if (!all_gen && !any_streamed && (double)m * (double)n * (double)n * 8.0 <= 16e9) {
            std::vector<double> gP((size_t)m * n * n, 0.0);
            for (int64_t k = 0; k < m; k++) {
                const HostQuad &h = c->quads[(size_t)k + 1];
                for (size_t e = 0; e < h.cv.size(); e++) gP[((size_t)k * n + h.ci[e]) * n + h.cj[e]] += h.cv[e];
            }
            const double *tmp = nullptr;
            if ((rc = prob_upload(c, &tmp, gP))) return rc;
            c->d_gP = const_cast<double *>(tmp);
            HIPCHK(c, spin_sync(c->stream));
        }
        if ((rc = prob_upload(c, &dp.gptr, gptr))) return rc;
        if ((rc = prob_upload(c, &dp.gi, gi))) return rc;
        if ((rc = prob_upload(c, &dp.gj, gj))) return rc;
        if ((rc = prob_upload(c, &dp.gv, gv))) return rc;
        if ((rc = prob_upload(c, &dp.gq, gq))) return rc;
        if ((rc = prob_upload(c, &dp.gr, gr))) return rc;
        if ((rc = prob_upload(c, &dp.grel, grel))) return rc;
        if ((c->d_gP || all_gen || any_streamed) && (double)(m + 1) * (double)n16 * (double)n16 * 8.0 <= 200e9 && (rc = dense_build(c, gq, gr, grel))) return rc;
        if (c->dn_force && !c->dn_Gpack) return fail(c, QCQPMI_EUNSUPPORTED, "generated functions need the dense path (matrices exceed 200 GB, or generated and uploaded coupled constraints are mixed beyond 16 GB)");
    }
    HIPCHK(c, c->d_best_idx.reserve(c->stream, 2));
    HIPCHK(c, c->d_best_key.reserve(c->stream, 2));
    HIPCHK(c, spin_sync(c->stream));
    // host copies are no longer needed
    for (auto &h : c->quads) { std::vector<int>().swap(h.ci); std::vector<int>().swap(h.cj); std::vector<double>().swap(h.cv); }
    c->finalized = true;
    return 0;
}

int qcqpmi_sdr_solve_unitdiag(qcqpmi_ctx *c, const double *C, int64_t N, double *V, int max_sweeps, double tol,
                              double *hist, int *sweeps_done) {
    if (!c) return QCQPMI_EINVAL;
    if (!C || !V || !hist || !sweeps_done || N < 2 || max_sweeps < 0 || !(tol >= 0.0))
        return fail(c, QCQPMI_EINVAL, "sdr_solve_unitdiag: bad arguments");
    if (N > SDR_NMAX) return fail(c, QCQPMI_EUNSUPPORTED, "sdr_solve_unitdiag: N = %lld exceeds %d", (long long)N, SDR_NMAX);
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<double> bC, bV, bh;
    DevBuf<int> bs;
    DevBuf<SdrWork> bw;
    HIPCHK(c, bC.reserve(c->stream, (size_t)N * N, false));
    HIPCHK(c, bV.reserve(c->stream, (size_t)N * SDR_K, false));
    HIPCHK(c, bh.reserve(c->stream, (size_t)max_sweeps + 2));
    HIPCHK(c, bs.reserve(c->stream, 1));
    HIPCHK(c, bw.reserve(c->stream, 1));      // zeroed: arrival counter, abort flag
    int sw = 0;
    HIPCHK(c, hipMemcpyAsync(bC.p, C, (size_t)N * N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(bV.p, V, (size_t)N * SDR_K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    {
        // 64 single-wave workgroups that synchronise through memory: cooperative launch = co-residency guaranteed
        // (the argument array holds ADDRESSES of the arguments: plain pointers, not the buffers)
        const double *aC = bC.p;
        double *dV = bV.p, *dh = bh.p;
        int *ds = bs.p;
        SdrWork *dw = bw.p;
        int aN = (int)N;
        void *args[] = {(void *)&aC, (void *)&dV, (void *)&aN, (void *)&max_sweeps, (void *)&tol, (void *)&dh, (void *)&ds, (void *)&dw};
        HIPCHK(c, hipLaunchCooperativeKernel((const void *)sdr_mixing_kernel, dim3(SDR_K), dim3(64), args,
                                             (unsigned)(2 * (size_t)N * sizeof(double)), c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(V, bV.p, (size_t)N * SDR_K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hist, bh.p, ((size_t)max_sweeps + 2) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&sw, bs.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    if (sw < 0) return fail(c, QCQPMI_EHIP, "sdr_solve_unitdiag: the workgroups lost step (spin limit reached)");
    *sweeps_done = sw;
    return 0;
}

int qcqpmi_is_separable(const qcqpmi_ctx *c) { return (c && c->finalized && c->sep) ? 1 : 0; }

// -------------------------------------------------------------------------------- population

int qcqpmi_pop_upload(qcqpmi_ctx *c, const double *X, int64_t R) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!X) return fail(c, QCQPMI_EINVAL, "pop_upload: X is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = pop_reserve(c, R))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_stage, X, (size_t)R * c->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    int64_t total = c->Rpad * c->n16;
    hipLaunchKernelGGL(to_tiles_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream,
                       c->d_stage, c->X, c->n, c->n16, R, c->Rpad);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

int qcqpmi_pop_download(qcqpmi_ctx *c, double *X, int64_t R) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!X || R <= 0 || R > c->R) return fail(c, QCQPMI_EINVAL, "pop_download: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    int64_t total = R * c->n;
    launch_from_tiles(c, c->X, R);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(X, c->d_stage, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

int64_t qcqpmi_pop_size(const qcqpmi_ctx *c) { return c ? c->R : 0; }

int qcqpmi_pop_randn(qcqpmi_ctx *c, int64_t R, uint64_t seed, uint64_t first_index) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = pop_reserve(c, R))) return rc;
    int64_t total = c->Rpad * c->n16;
    hipLaunchKernelGGL(randn_tiles_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream,
                       c->X, c->n, c->n16, R, c->Rpad, seed, first_index);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int qcqpmi_pop_sdr_sample(qcqpmi_ctx *c, const double *mu, const double *F, int64_t S, uint64_t seed,
                          uint64_t first_index, const double *Xi) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    // mu == NULL && F == NULL: the factor and mean of the previous call are still resident (packed for the matrix cores)
    const bool reuse = !mu && !F;
    if (!reuse && (!mu || !F)) return fail(c, QCQPMI_EINVAL, "pop_sdr_sample: mu / F missing (both NULL = reuse the previous pair)");
    if (reuse && !c->sdr_factor_resident) return fail(c, QCQPMI_ESTATE, "pop_sdr_sample: no resident factor to reuse");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->n, n16 = c->n16;
    HIPCHK(c, c->d_Fpack.reserve(c->stream, (size_t)n16 * n16));
    HIPCHK(c, c->d_Frow.reserve(c->stream, (size_t)n16 * n16));
    HIPCHK(c, c->d_mu.reserve(c->stream, (size_t)n16));
    if (!reuse) {
        HIPCHK(c, hipMemsetAsync(c->d_Frow, 0, (size_t)n16 * n16 * sizeof(double), c->stream));
        HIPCHK(c, hipMemcpy2DAsync(c->d_Frow, (size_t)n16 * sizeof(double), F, (size_t)n * sizeof(double),
                                   (size_t)n * sizeof(double), (size_t)n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_mu, mu, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        int64_t total = n16 * n16;
        hipLaunchKernelGGL(pack_A_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream,
                           c->d_Frow, c->d_Fpack, n16, c->dp.KS);
        c->sdr_factor_resident = true;
        // the 2D copy may pin the caller's pages and return with the DMA in flight; the caller (Engine.sdr_sample passes
        // temporaries) may free F / mu as soon as this call returns.  The reuse path (mu = F = NULL) stays asynchronous.
        HIPCHK(c, spin_sync(c->stream));
    }
    if ((rc = pop_reserve(c, S))) return rc;
    // the standard normals: caller-provided (host layout) or device Philox; the buffer is kept across calls
    HIPCHK(c, c->Xi.reserve(c->stream, (size_t)c->Rpad * n16, false));
    int64_t tot2 = c->Rpad * n16;
    if (Xi) {
        HIPCHK(c, hipMemcpyAsync(c->d_stage, Xi, (size_t)S * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(to_tiles_kernel, dim3((unsigned)((tot2 + 255) / 256)), dim3(256), 0, c->stream,
                           c->d_stage, c->Xi, n, n16, S, c->Rpad);
    } else {
        hipLaunchKernelGGL(randn_tiles_kernel, dim3((unsigned)((tot2 + 255) / 256)), dim3(256), 0, c->stream,
                           c->Xi, n, n16, S, c->Rpad, seed, first_index);
    }
    tic(c, 3);
    if (c->dp.NB >= 8 && c->Rpad / 16 >= 8) {
        // x = mu + F xi as one LDS-tiled MFMA GEMM (8 row blocks of F x 8 tiles of samples per workgroup)
        if ((rc = launch_dense_product(c, 3, c->d_Fpack, c->d_mu, c->Xi, c->X))) return rc;
    } else {
        hipLaunchKernelGGL(affine_tiles_kernel, dim3((unsigned)(c->Rpad / 16)), dim3(256), 0, c->stream,
                           c->d_Fpack, c->d_mu, c->Xi, c->X, n, n16, c->dp.NB, c->dp.KS);
    }
    toc(c, 3);
    HIPCHK(c, hipGetLastError());
    // F / mu were synchronised above; a caller-provided Xi went through a pageable 1D copy (host-synchronous staging).  The
    // samples are in stream order for whatever comes next (evaluation, download); no synchronisation here.
    return 0;
}

// --------------------------------------------------------------------------------- evaluation

int qcqpmi_pop_eval(qcqpmi_ctx *c, double *f0, double *maxviol, double *F) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = launch_eval(c, F != nullptr))) return rc;
    if (f0) HIPCHK(c, hipMemcpyAsync(f0, c->d_f0, (size_t)c->R * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (maxviol) HIPCHK(c, hipMemcpyAsync(maxviol, c->d_mv, (size_t)c->R * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (F)
        HIPCHK(c, hipMemcpy2DAsync(F, (size_t)c->R * sizeof(double), c->d_F, (size_t)c->Rpad * sizeof(double),
                                   (size_t)c->R * sizeof(double), (size_t)(c->m + 1), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

// ---- suggest(SDR) for S samples in one call (qcqp.py:396-401: x = multivariate_normal(mu, Sigma), f0.eval(x), max(violations(x));
// SURVEY section 8b's qcqpmi_sdr_sample_eval).  The samples are drawn (x = mu + F xi, normals by keyed Philox: sample first_index + s
// is the same point whatever S and the chunking) and evaluated chunk by chunk on the stream: the normals and the points of a chunk
// live in two buffers every chunk reuses (<= 32 MB each, sized to fit the 256 MB Infinity Cache between the sampler's GEMM and the
// evaluation's GEMM; not measured separately: at configs[2]'s size the round trip of X is 1 % of the two GEMMs either way); a
// population of S points is never laid out in HBM.  X_opt == NULL: the points are not kept at all -- the caller
// re-draws the winner from its index (S = 1, the same first_index + s).  Afterwards the resident population is the LAST chunk.
int qcqpmi_sdr_sample_eval(qcqpmi_ctx *c, const double *mu, const double *F, int64_t S, uint64_t seed, uint64_t first_index,
                           double *X_opt, double *f0, double *maxviol) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (S < 1 || !f0 || !maxviol) return fail(c, QCQPMI_EINVAL, "sdr_sample_eval: S < 1 or f0 / maxviol missing");
    int64_t chunk = ((int64_t)32 << 20) / (c->n16 * (int64_t)sizeof(double));
    chunk = chunk / 128 * 128;                       // whole groups of 8 tiles of 16 samples (the LDS-tiled GEMMs' unit)
    if (chunk < 128) chunk = 128;
    if (const char *ev = getenv("QCQPMI_SDR_CHUNK")) { const int64_t v = atoll(ev); if (v >= 16) chunk = v / 16 * 16; }     // tests: several chunks at small sizes
    for (int64_t off = 0; off < S; off += chunk) {
        const int64_t cnt = S - off < chunk ? S - off : chunk;
        if ((rc = qcqpmi_pop_sdr_sample(c, off == 0 ? mu : nullptr, off == 0 ? F : nullptr, cnt, seed, first_index + (uint64_t)off, nullptr))) return rc;
        if ((rc = launch_eval(c, false))) return rc;
        HIPCHK(c, hipMemcpyAsync(f0 + off, c->d_f0, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(maxviol + off, c->d_mv, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (X_opt) {
            if ((rc = qcqpmi_pop_download(c, X_opt + off * c->n, cnt))) return rc;
        }
    }
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

int qcqpmi_get_linear(qcqpmi_ctx *c, int64_t k, double *q, double *r, int *relop) {
    if (!c) return QCQPMI_EINVAL;
    if (k < 0 || k > c->m || !c->quads[(size_t)k].set) return fail(c, QCQPMI_EINVAL, "get_linear: bad k");
    const HostQuad &h = c->quads[(size_t)k];
    if (q) memcpy(q, h.q.data(), (size_t)c->n * sizeof(double));
    if (r) *r = h.r;
    if (relop) *relop = h.relop;
    return 0;
}

int qcqpmi_eval_batch(qcqpmi_ctx *c, const double *X, int64_t S, double *f0, double *maxviol, double *F) {
    int rc = qcqpmi_pop_upload(c, X, S);
    if (rc) return rc;
    return qcqpmi_pop_eval(c, f0, maxviol, F);
}

// -------------------------------------------------------------------------------- best of pop

int qcqpmi_select_best(qcqpmi_ctx *c, double tol, int64_t *best_index, double *best_f0,
                       double *best_maxviol, double *best_x) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->evaluated && (rc = launch_eval(c, false))) return rc;
    launch_select_best(c, 1, c->d_f0, c->d_mv, c->R, tol, c->d_best_idx, c->d_best_key);
    HIPCHK(c, hipGetLastError());
    int64_t idx[2];
    double key[2];
    HIPCHK(c, hipMemcpyAsync(idx, c->d_best_idx, sizeof(idx), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(key, c->d_best_key, sizeof(key), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    if (best_index) *best_index = idx[0];
    if (best_f0) *best_f0 = key[0];
    if (best_maxviol) *best_maxviol = key[1];
    if (best_x && idx[0] >= 0) {
        int64_t r = idx[0];
        const double *src = c->X + (r >> 4) * c->n16 * 16 + (r & 15);
        HIPCHK(c, hipMemcpy2DAsync(best_x, sizeof(double), src, 16 * sizeof(double), sizeof(double), (size_t)c->n,
                                   hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, spin_sync(c->stream));
    }
    return 0;
}

const char *qcqpmi_last_cd_kernel(qcqpmi_ctx *c) { return c ? c->last_cd2_kernel : ""; }

int qcqpmi_last_kernel_ms(qcqpmi_ctx *c, int which, double *ms) {
    if (!c || which < 0 || which > 4 || !ms) return QCQPMI_EINVAL;
    if (!c->timers[which].valid) return fail(c, QCQPMI_ESTATE, "kernel %d has not been launched", which);
    HIPCHK(c, hipEventSynchronize(c->timers[which].end));
    float f = 0.f;
    HIPCHK(c, hipEventElapsedTime(&f, c->timers[which].beg, c->timers[which].end));
    *ms = (double)f;
    return 0;
}

int qcqpmi_sync(qcqpmi_ctx *c) {
    if (!c) return QCQPMI_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

}  // extern "C"

