// C ABI of libqcqp_mi.so, the dense-constraint path (cd_dense.h, cd_dense_mw.h; this unit alone compiles their kernels): packing
// at upload and finalize, MFMA evaluation of all m+1 functions, the sweep / block loops of coordinate descent, and the operators
// of the relaxation solver on the packed matrices (weighted sum, weighted product, quadratic and linear parts).  The LDS-tiled
// GEMM of cd_dense.h also multiplies ONE packed matrix with the population for the core (launch_dense_product).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "capi_ctx.h"
#include "cd_dense_mw.h"      // with it cd_dense.h

using namespace qcqpmi;

namespace {

// which chain kernel the dense path dispatches to (four waves per restart unless a thread would hold more than 8 slots)
bool dense_chain_mw(const qcqpmi_ctx *c) { return c->dense_chain_mode != 1 && mw_geometry((int)c->m + 1).SL <= 8; }

DenseProblem dense_problem(const qcqpmi_ctx *c) {
    DenseProblem D;
    D.Gpack = c->dn_Gpack; D.q = c->dn_q; D.r = c->dn_r; D.relop = c->dn_relop;
    D.qT = c->dn_qT;
    D.n = c->n; D.n16 = c->n16; D.NB = (int)(c->n16 / 16); D.KS = (int)(c->n16 / 4); D.m1 = (int)c->m + 1;
    D.m1p = (D.m1 + 63) / 64 * 64;
    return D;
}

// pinned host memory for downloads that are repeated thousands of times (a 2-D copy into pageable memory is staged row by
// row by the runtime: 1025 rows of 47 doubles cost 15 ms)
int pin_reserve(qcqpmi_ctx *c, size_t bytes) {
    HIPCHK(c, c->h_pin.reserve(c->stream, bytes, false));
    return 0;
}

}  // namespace

namespace qcqpmi {

bool dense_on(const qcqpmi_ctx *c) { return !c->sep && c->dn_Gpack && (c->n > 64 || c->dn_force || (c->dbg & 32)); }

const char *dense_chain_name(const qcqpmi_ctx *c) { return dense_chain_mw(c) ? "dense_chain_mw_kernel" : "dense_chain_kernel"; }

// (dense_pack_kernel addresses function k at gP + (k - 1) n n: hand it a base that puts the staging buffer there)
void launch_dense_pack_staged(qcqpmi_ctx *c, int64_t k, double *gpack) {
    const int64_t n = c->n, n16 = c->n16, total = n16 * n16;
    hipLaunchKernelGGL(dense_pack_kernel, dim3((unsigned)((total + 255) / 256), 1), dim3(256), 0, c->stream, (const double *)nullptr,
                       (const double *)(c->dn_tmp - (k - 1) * n * n), gpack, n, n16, (int)(c->m + 1), (int)k);
}

void launch_dense_gen_rowmajor(qcqpmi_ctx *c, double *P, int k, uint64_t seed, double scale, double diag_add) {
    const int64_t n16 = c->n16;
    hipLaunchKernelGGL(dense_gen_rowmajor_kernel, dim3((unsigned)((n16 * n16 + 255) / 256)), dim3(256), 0, c->stream, P, c->n, n16, k, seed,
                       scale, diag_add);
}

// finalize: every matrix into the block-major fragment layout
int dense_build(qcqpmi_ctx *c, const std::vector<double> &gq, const std::vector<double> &gr, const std::vector<int> &grel) {
    const int64_t n = c->n, n16 = c->n16, m1 = c->m + 1;
    int rc;
    double *gp = nullptr;
    if (c->dn_gp_pre) {             // streaming upload: the constraint matrices are packed already (qcqpmi_set_quad)
        const size_t bytes = c->dn_gp_pre.cap * sizeof(double);
        gp = c->dn_gp_pre.take();
        c->prob_allocs.emplace_back((char *)gp, bytes);
    } else if ((rc = prob_alloc(c, &gp, (size_t)m1 * n16 * n16))) return rc;
    const int64_t total = n16 * n16;
    const unsigned pb = (unsigned)((total + 255) / 256);
    // function 0 from the row-major P0 (uploaded or generated), the others from gP or from the generator
    hipLaunchKernelGGL(dense_pack_kernel, dim3(pb, 1), dim3(256), 0, c->stream, c->dp.P0, c->d_gP, gp, n, n16, (int)m1, 0);
    for (int64_t k = 1; k < m1; k++) {
        const HostQuad &h = c->quads[(size_t)k];
        if (h.streamed) continue;
        if (h.gen)
            hipLaunchKernelGGL(dense_gen_pack_kernel, dim3(pb), dim3(256), 0, c->stream, gp, n, n16, (int)m1, (int)k, h.gseed, h.gscale, h.gdiag);
        else if (c->d_gP)
            hipLaunchKernelGGL(dense_pack_kernel, dim3(pb, 1), dim3(256), 0, c->stream, c->dp.P0, c->d_gP, gp, n, n16, (int)m1, (int)k);
        else {
            // streaming mode (no row-major copy of the constraint matrices exists) and this function was not streamed by
            // qcqpmi_set_quad because it touches a single coordinate (a box constraint x_i^2 <= 1 among coupled ones) or
            // none: pack it now from the host triplets through the staging buffer
            HIPCHK(c, c->dn_tmp.reserve(c->stream, (size_t)n * n, false));
            std::vector<double> dense((size_t)n * n, 0.0);
            for (size_t e = 0; e < h.cv.size(); e++) dense[(size_t)h.ci[e] * n + h.cj[e]] += h.cv[e];
            HIPCHK(c, hipMemcpyAsync(c->dn_tmp, dense.data(), (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
            launch_dense_pack_staged(c, k, gp);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, spin_sync(c->stream));      // the staging buffer is free again
        }
    }
    HIPCHK(c, hipGetLastError());
    std::vector<double> q((size_t)m1 * n16, 0.0), r((size_t)m1, 0.0);
    std::vector<int> rel((size_t)m1, 0);
    for (int64_t j = 0; j < n; j++) q[(size_t)j] = c->quads[0].q[(size_t)j];
    r[0] = c->quads[0].r;
    for (int64_t k = 1; k < m1; k++) {
        memcpy(&q[(size_t)k * n16], &gq[(size_t)(k - 1) * n16], (size_t)n16 * sizeof(double));
        r[(size_t)k] = gr[(size_t)k - 1];
        rel[(size_t)k] = grel[(size_t)k - 1];
    }
    const int64_t m1p = (m1 + 63) / 64 * 64;
    std::vector<double> qT((size_t)n16 * m1p, 0.0);
    for (int64_t k = 0; k < m1; k++)
        for (int64_t j = 0; j < n; j++) qT[(size_t)j * m1p + k] = q[(size_t)k * n16 + j];
    const double *tq = nullptr, *tr = nullptr, *tqT = nullptr;
    const int *trel = nullptr;
    if ((rc = prob_upload(c, &tq, q))) return rc;
    if ((rc = prob_upload(c, &tqT, qT))) return rc;
    if ((rc = prob_upload(c, &tr, r))) return rc;
    if ((rc = prob_upload(c, &trel, rel))) return rc;
    HIPCHK(c, spin_sync(c->stream));
    c->dn_tmp.release();      // no function arrives after finalize
    c->dn_Gpack = gp; c->dn_q = tq; c->dn_qT = tqT; c->dn_r = tr; c->dn_relop = trel;
    return 0;
}

}  // namespace qcqpmi

namespace {

// grid.z of the products kernel (K-split of the contraction) when functions x tiles alone do not fill the chip's 512
// workgroup slots (2 per CU): the split that minimises rounds of workgroups per unit of work, with a small charge per plane
// (every plane is written once and read once by the chain).  m + 1 = 257 functions are 33 groups of 8: a split of 4 would
// need 528 slots -- a second round for 16 workgroups, 50 % longer -- where 3 needs 396.
int dense_zsplit(int m1, int ntiles, int limit) {
    const int64_t wg = (int64_t)((m1 + DP_FG - 1) / DP_FG) * ((ntiles + DP_TG - 1) / DP_TG);
    int zs = 1;
    if (wg < 512) {
        double best = 1e30;
        for (int z = 1; z <= 7; z++) {   // 7 + the fix-up plane = the 8 planes the chain sums
            const double cost = (double)((wg * z + 511) / 512) / z + 0.02 * z;
            if (cost < best - 1e-12) { best = cost; zs = z; }
        }
    }
    if (const char *e = getenv("QCQPMI_DENSE_ZS")) zs = atoi(e);      // experiments
    zs = std::min(std::min(zs, 7), limit);
    return std::max(zs, 1);
}

}  // namespace

namespace qcqpmi {

int dense_product_planes(int NB) { return 2 * ((NB + DP_FG - 1) / DP_FG); }

// ONE matrix times the population through the LDS-tiled GEMM (8 row blocks x 8 tiles per workgroup share their operands).
// mode 2: x'Mx, one partial plane per wave row of a group of row blocks (launch_eval: M = the packed P0; the per-tile MFMA loop of
// eval_kernel re-reads all of P0 from L2 for every tile); mode 3: OUT = mu 1' + M X (qcqpmi_pop_sdr_sample: x = mu + F xi;
// qcqpmi_pop_weighted_product: Y = S X with a zero mu).  The kernel reads Gpack, q, n, n16, NB, KS of the problem in these modes.
int launch_dense_product(qcqpmi_ctx *c, int mode, const double *Mpack, const double *mu, const double *X, double *out) {
    DenseProdArgs pa;
    pa.D.Gpack = Mpack; pa.D.q = mu; pa.D.qT = nullptr; pa.D.r = nullptr; pa.D.relop = nullptr;
    pa.D.n = c->n; pa.D.n16 = c->n16; pa.D.NB = (int)(c->n16 / 16); pa.D.KS = (int)(c->n16 / 4); pa.D.m1 = 1; pa.D.m1p = 64;
    pa.X = X; pa.ntiles = (int)(c->Rpad / 16); pa.b = 0; pa.zs = 1; pa.G = mode == 3 ? out : nullptr; pa.F = mode == 2 ? out : nullptr;
    pa.Rpad = c->Rpad; pa.tile_on = nullptr; pa.hole = -1; pa.ch_only = -1; pa.zplane = 0;
    auto kg = mode == 2 ? dense_products_kernel<2> : dense_products_kernel<3>;
    HIPCHK(c, hipFuncSetAttribute((const void *)kg, hipFuncAttributeMaxDynamicSharedMemorySize, DP_LDS_BYTES));
    hipLaunchKernelGGL(kg, dim3((unsigned)((pa.D.NB + DP_FG - 1) / DP_FG), (unsigned)((pa.ntiles + DP_TG - 1) / DP_TG), 1), dim3(256),
                       DP_LDS_BYTES, c->stream, pa);
    return 0;
}

// all function values on the matrix cores, then f0 / max violation per candidate
int launch_eval_dense(qcqpmi_ctx *c, bool with_Ft) {
    DenseProdArgs a;
    a.D = dense_problem(c);
    a.ntiles = (int)(c->Rpad / 16);
    a.zs = dense_zsplit(a.D.m1, a.ntiles, a.D.NB);
    HIPCHK(c, c->d_F.reserve(c->stream, (size_t)((int64_t)(a.zs + 1) * (c->m + 1) * c->Rpad)));   // partial planes + the linear terms
    a.X = c->X; a.b = 0; a.G = nullptr; a.F = c->d_F; a.Rpad = c->Rpad; a.tile_on = nullptr;
    a.hole = -1; a.ch_only = -1; a.zplane = 0;
    auto k = dense_products_kernel<1>;
    HIPCHK(c, hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, DP_LDS_BYTES));
    tic(c, 0);
    hipLaunchKernelGGL(k, dim3((unsigned)((a.D.m1 + DP_FG - 1) / DP_FG), (unsigned)((a.ntiles + DP_TG - 1) / DP_TG), (unsigned)a.zs),
                       dim3(256), DP_LDS_BYTES, c->stream, a);
    double *lin = c->d_F + (int64_t)a.zs * (c->m + 1) * c->Rpad;
    hipLaunchKernelGGL(dense_linear_kernel, dim3((unsigned)a.ntiles, (unsigned)((a.D.m1 + 15) / 16)), dim3(256), 0, c->stream,
                       a.D, (const double *)c->X, c->Rpad, lin);
    hipLaunchKernelGGL(dense_viol_kernel, dim3((unsigned)((c->Rpad + 255) / 256)), dim3(256), 0, c->stream,
                       c->d_F, a.zs, (const double *)lin, c->dn_relop, a.D.m1, a.D.m1p, c->Rpad, c->d_f0, c->d_mv, with_Ft ? c->dn_Ft : (double *)nullptr);
    toc(c, 0);
    HIPCHK(c, hipGetLastError());
    c->evaluated = true;
    return 0;
}

}  // namespace qcqpmi

namespace {

// quadratic parts x'P_k x + r_k (plane 0 of d_F) and linear parts q_k'x (the plane after the partial planes) of all
// functions, kept separate: the homogeneous forms of the SDP solver need them apart
int eval_parts_dense(qcqpmi_ctx *c) {
    DenseProdArgs a;
    a.D = dense_problem(c);
    a.ntiles = (int)(c->Rpad / 16);
    a.zs = dense_zsplit(a.D.m1, a.ntiles, a.D.NB);
    c->eval_zs = a.zs;
    HIPCHK(c, c->d_F.reserve(c->stream, (size_t)((int64_t)(a.zs + 1) * (c->m + 1) * c->Rpad)));
    a.X = c->X; a.b = 0; a.G = nullptr; a.F = c->d_F; a.Rpad = c->Rpad; a.tile_on = nullptr;
    a.hole = -1; a.ch_only = -1; a.zplane = 0;
    auto k = dense_products_kernel<1>;
    HIPCHK(c, hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, DP_LDS_BYTES));
    hipLaunchKernelGGL(k, dim3((unsigned)((a.D.m1 + DP_FG - 1) / DP_FG), (unsigned)((a.ntiles + DP_TG - 1) / DP_TG), (unsigned)a.zs),
                       dim3(256), DP_LDS_BYTES, c->stream, a);
    double *lin = c->d_F + (int64_t)a.zs * (c->m + 1) * c->Rpad;
    hipLaunchKernelGGL(dense_linear_kernel, dim3((unsigned)a.ntiles, (unsigned)((a.D.m1 + 15) / 16)), dim3(256), 0, c->stream,
                       a.D, (const double *)c->X, c->Rpad, lin);
    const int64_t tot = (int64_t)a.D.m1 * c->Rpad;
    hipLaunchKernelGGL(dense_sum_planes_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, c->d_F, a.zs, a.D.m1, c->Rpad);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int dense_reserve(qcqpmi_ctx *c) {
    const int64_t ntiles = c->Rpad / 16, m1 = c->m + 1, m1p = (m1 + 63) / 64 * 64;
    // two buffers (block b is read while b+1 is produced), each: K-split planes + the fix-up plane
    const int64_t gneed = 2 * (int64_t)(dense_zsplit((int)m1, (int)ntiles, (int)(c->n16 / 16)) + 1) * ntiles * 256 * m1p;
    HIPCHK(c, c->dn_G.reserve(c->stream, (size_t)gneed, false));
    HIPCHK(c, c->dn_Ft.reserve(c->stream, (size_t)(c->Rpad * m1p)));
    HIPCHK(c, c->dn_Dg.reserve(c->stream, (size_t)m1p * 512));
    if (c->profile) HIPCHK(c, c->dn_prof.reserve(c->stream, 64));      // (zeroed once; qcqpmi_debug_dense_profile reads and clears)
    if (!c->stream2) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
        for (auto &e : c->dn_ev) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (auto &e : c->dn_evn) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    HIPCHK(c, c->dn_hn.reserve(c->stream, 2, false));
    // upd, viol_last (8 B each) + live, on, tile_on (1 B each) + nlive
    HIPCHK(c, c->dn_state.reserve(c->stream, (size_t)c->Rpad * (8 + 8 + 1 + 1 + 1) + 64, false));
    return 0;
}

DenseState dense_state(qcqpmi_ctx *c, bool phase1) {
    DenseState S;
    char *p = c->dn_state;
    const size_t Rp = (size_t)c->Rpad;      // (every phase lays the buffer out afresh: dense_state_init_kernel)
    S.upd = (int64_t *)p; p += Rp * 8;
    S.viol_last = (double *)p; p += Rp * 8;
    S.nlive = (int *)p; p += 64;
    S.live = (uint8_t *)p; p += Rp;
    S.on = (uint8_t *)p; p += Rp;
    S.tile_on = (uint8_t *)p;
    S.visits = c->d_visits; S.accepted = c->d_acc;
    S.sweeps = phase1 ? c->d_sweeps1 : c->d_sweeps;
    S.status = phase1 ? c->d_status1 : c->d_status;
    return S;
}

// one phase: sweeps over the blocks until no restart is live.  The host runs ONE SWEEP AHEAD of the device: the live count of
// sweep t travels to pinned memory behind an event, the blocks of sweep t are enqueued without waiting for it (with nothing
// live they are empty launches: tile flags), and it is looked at before sweep t + 1 is enqueued -- no synchronisation stalls
// the stream; one sweep of empty launches per phase is the price.
// only_block >= 0 (qcqpmi_cd_dense_block_step, the teacher-forced unit step of the parity tests): ONE launch sequence --
// products of that block over the full contraction, diagonal blocks, chain -- as sweep number t_first of the keyed stream.
template <int PHASE>
int dense_phase(qcqpmi_ctx *c, int64_t num_iters, double viol_tol, double tol, uint64_t seed, uint64_t first_index,
                int64_t t_first = 0, int only_block = -1, int c_lo = 0, int c_hi = 16) {
    const int ntiles = (int)(c->Rpad / 16);
    const DenseProblem D = dense_problem(c);
    DenseState S = dense_state(c, PHASE == 1);
    const unsigned rb = (unsigned)((c->Rpad + 255) / 256);
    hipLaunchKernelGGL(dense_state_init_kernel, dim3(rb), dim3(256), 0, c->stream, S, PHASE == 2 ? c->d_flag : (const uint8_t *)nullptr, c->R, c->Rpad);
    DenseProdArgs pa;
    pa.D = D; pa.X = c->X; pa.ntiles = ntiles; pa.G = c->dn_G; pa.F = nullptr; pa.Rpad = c->Rpad; pa.tile_on = S.tile_on;
    pa.zs = dense_zsplit(D.m1, ntiles, D.NB);
    DenseChainArgs ca;
    ca.D = D; ca.X = c->X; ca.R = c->R; ca.Rpad = c->Rpad; ca.G = c->dn_G; ca.Dg = c->dn_Dg; ca.Ft = c->dn_Ft;
    ca.zs = pa.zs; ca.gz_stride = (int64_t)ntiles * 256 * D.m1p;
    // chain kernel: four waves per restart (cd_dense_mw.h) unless there are more than 8 function slots per thread or the
    // one-wave kernel was asked for (qcqpmi_dense_chain_mode: the cross-check)
    const MwGeom mg = mw_geometry(D.m1);
    const int mw_sl = mg.SL, mw_T = mg.T;
    ca.mw_Tc = mg.Tc; ca.mw_ts = mg.ts;
    const bool mw = dense_chain_mw(c);
    // one-wave kernel: restarts per workgroup / staging of G in LDS: whatever fits 160 KB
    const size_t per_small = (DN_FARR_MIN * (size_t)D.m1p + DN_LDS_WAVE) * sizeof(double), per_big = ((16 + DN_FARR) * (size_t)D.m1p + DN_LDS_WAVE) * sizeof(double);
    // staging G pays when the chip is not full of restarts anyway (it costs occupancy: 22 instead of 4 arrays per wave)
    const bool glds = per_big <= 160 * 1024 && c->R <= 1024;
    const size_t per = glds ? per_big : per_small;
    int wpb = DN_WPB;
    while (wpb > 1 && per * wpb > 160 * 1024) wpb--;
    const size_t lds = mw ? dense_chain_mw_lds_bytes(D.m1p) : per * wpb;
    if (lds > 160 * 1024) return fail(c, QCQPMI_EUNSUPPORTED, "coupled constraints: m = %d too large for the per-restart LDS tables", D.m1 - 1);
    // the one-wave kernel keeps one flag per function slot of a lane (DnSlotBits); the LDS tables end far below that today
    if (!mw && D.m1p > 64 * DN_SLOTS) return fail(c, QCQPMI_EUNSUPPORTED, "coupled constraints: m = %d beyond the %d function slots per lane of dense_chain_kernel", D.m1 - 1, DN_SLOTS);
    ca.prof = c->profile ? c->dn_prof : nullptr;
    ca.slack = c->d_mv; ca.S = S; ca.tol = tol; ca.viol_tol = viol_tol; ca.seed = seed; ca.first_index = first_index;
    void (*kc)(DenseChainArgs);
    if (mw) kc = mw_sl <= 1 ? dense_chain_mw_kernel<PHASE, 1> : mw_sl <= 2 ? dense_chain_mw_kernel<PHASE, 2> : mw_sl <= 4 ? dense_chain_mw_kernel<PHASE, 4> : dense_chain_mw_kernel<PHASE, 8>;
    else kc = glds ? dense_chain_kernel<PHASE, true> : dense_chain_kernel<PHASE, false>;
    HIPCHK(c, hipFuncSetAttribute((const void *)kc, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    auto kp = dense_products_kernel<0>;
    HIPCHK(c, hipFuncSetAttribute((const void *)kp, hipFuncAttributeMaxDynamicSharedMemorySize, DP_LDS_BYTES));
    const dim3 pgrid((unsigned)((D.m1 + DP_FG - 1) / DP_FG), (unsigned)((ntiles + DP_TG - 1) / DP_TG), (unsigned)pa.zs);
    const dim3 fgrid(pgrid.x, pgrid.y, 1);
    const dim3 cgrid(mw ? (unsigned)c->R : (unsigned)((c->R + wpb - 1) / wpb)), cblock(mw ? mw_T : 64 * wpb);
    const int64_t plane = (int64_t)ntiles * 256 * D.m1p;
    double *Gb[2] = {c->dn_G, c->dn_G + (int64_t)(pa.zs + 1) * plane};
    double *Db[2] = {c->dn_Dg, c->dn_Dg + (int64_t)256 * D.m1p};
    hipStream_t sA = c->stream, sB = c->stream2;
    hipEvent_t evStart = c->dn_ev[0], evChain = c->dn_ev[1], evProd = c->dn_ev[2];
    tic(c, PHASE);
    for (int64_t t = t_first; t < t_first + num_iters; t++) {
        if (t >= t_first + 1) {     // the count of the sweep enqueued last: long there unless the device is more than a sweep behind
            HIPCHK(c, hipEventSynchronize(c->dn_evn[(t - 1) & 1]));
            if (c->dn_hn[(t - 1) & 1] == 0) break;
        }
        HIPCHK(c, hipMemsetAsync(S.nlive, 0, sizeof(int), sA));
        hipLaunchKernelGGL(dense_sweep_begin_kernel<PHASE>, dim3((unsigned)((c->Rpad + 63) / 64)), dim3(64), 0, sA, S, c->R, c->Rpad, viol_tol);
        HIPCHK(c, hipMemcpyAsync(&c->dn_hn[t & 1], S.nlive, sizeof(int), hipMemcpyDeviceToHost, sA));
        HIPCHK(c, hipEventRecord(c->dn_evn[t & 1], sA));
        ca.t = t;
        if (only_block >= 0) {
            pa.b = only_block; pa.hole = -1; pa.ch_only = -1; pa.zplane = 0; pa.G = Gb[0];
            hipLaunchKernelGGL(kp, pgrid, dim3(256), DP_LDS_BYTES, sA, pa);
            hipLaunchKernelGGL(dense_diag_kernel, dim3((unsigned)D.m1), dim3(256), 0, sA, D, only_block, Db[0]);
            ca.b = only_block; ca.G = Gb[0]; ca.Dg = Db[0]; ca.zs = pa.zs; ca.c_lo = c_lo; ca.c_hi = c_hi;
            hipLaunchKernelGGL(kc, cgrid, cblock, lds, sA, ca);
            HIPCHK(c, hipGetLastError());
            break;
        }
        // Block 0: full contraction on the main stream.  Blocks b >= 1 are pipelined over two streams:
        // while the chain walks block b (main stream), the second stream already multiplies for block
        // b+1 -- without the 16 columns of block b, which the chain is rewriting; when the chain is
        // done a one-stage launch adds those columns into an extra plane (the "hole" trick of the
        // headline kernel, at kernel granularity).
        HIPCHK(c, hipEventRecord(evStart, sA));
        pa.b = 0; pa.hole = -1; pa.ch_only = -1; pa.zplane = 0; pa.G = Gb[0];
        hipLaunchKernelGGL(kp, pgrid, dim3(256), DP_LDS_BYTES, sA, pa);
        hipLaunchKernelGGL(dense_diag_kernel, dim3((unsigned)D.m1), dim3(256), 0, sA, D, 0, Db[0]);
        int nz = pa.zs;
        for (int b = 0; b < D.NB; b++) {
            const int cur = b & 1, nxt = cur ^ 1;
            const bool more = b + 1 < D.NB;
            if (more) {
                HIPCHK(c, hipStreamWaitEvent(sB, b == 0 ? evStart : evChain, 0));   // chain(b-1) done: X final outside block b, buffer nxt free
                pa.b = b + 1; pa.hole = b; pa.ch_only = -1; pa.zplane = 0; pa.G = Gb[nxt];
                hipLaunchKernelGGL(kp, pgrid, dim3(256), DP_LDS_BYTES, sB, pa);
                hipLaunchKernelGGL(dense_diag_kernel, dim3((unsigned)D.m1), dim3(256), 0, sB, D, b + 1, Db[nxt]);
                HIPCHK(c, hipEventRecord(evProd, sB));
            }
            ca.b = b; ca.G = Gb[cur]; ca.Dg = Db[cur]; ca.zs = nz;
            hipLaunchKernelGGL(kc, cgrid, cblock, lds, sA, ca);
            if (more) {
                HIPCHK(c, hipEventRecord(evChain, sA));
                HIPCHK(c, hipStreamWaitEvent(sA, evProd, 0));
                pa.b = b + 1; pa.hole = -1; pa.ch_only = b; pa.zplane = pa.zs; pa.G = Gb[nxt];
                hipLaunchKernelGGL(kp, fgrid, dim3(256), DP_LDS_BYTES, sA, pa);
                nz = pa.zs + 1;
            }
        }
        if (PHASE == 1)
            hipLaunchKernelGGL(dense_sweep_end_kernel, dim3(rb), dim3(256), 0, c->stream, S, (const double *)c->dn_Ft, c->dn_relop, D.m1, D.m1p, c->R);
        HIPCHK(c, hipGetLastError());
    }
    toc(c, PHASE);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// debug: stage tick sums of the chain kernel's wave of restart 0 since the profile was enabled ([0..15] phase 1,
// [16..31] phase 2 of the serial thread / the one-wave kernel's wave, [32..63] the same for thread 0 of the multi-wave
// kernel; slots: DnProf in cd_dense.h); reading resets them
int dense_profile_read(qcqpmi_ctx *c, int64_t *out64) {
    for (int k = 0; k < 64; k++) out64[k] = 0;
    if (!c->dn_prof) return 0;
    HIPCHK(c, spin_sync(c->stream));
    HIPCHK(c, hipMemcpy(out64, c->dn_prof, 64 * sizeof(long long), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemset(c->dn_prof, 0, 64 * sizeof(long long)));
    return 0;
}

// qcqpmi_cd_dense_block_step: the unit step of the dense path -- what one (sweep, block) iteration of dense_phase does to
// the resident points, started from FRESH function values (and, for phase 2, from the slack the caller passes: the
// reference fixes it once per phase, qcqp.py:157).  The parity tests drive it with the states the oracle visits.
int cd_dense_block_step(qcqpmi_ctx *c, int phase, int64_t sweep, int64_t block, int coord_lo, int coord_hi, double viol_tol, double tol,
                        uint64_t seed, uint64_t first_index, const double *slack) {
    if ((phase != 1 && phase != 2) || sweep < 0 || block < 0 || block >= c->n16 / 16 || !(tol > 0.0) || coord_lo < 0 || coord_hi > 16 || coord_lo >= coord_hi)
        return fail(c, QCQPMI_EINVAL, "cd_dense_block_step: phase %d, sweep %lld, block %lld, coordinates [%d, %d)", phase, (long long)sweep, (long long)block, coord_lo, coord_hi);
    if ((coord_lo != 0 || coord_hi != 16) && !dense_chain_mw(c))
        return fail(c, QCQPMI_EUNSUPPORTED, "cd_dense_block_step: a coordinate range needs dense_chain_mw_kernel (this problem / mode takes the one-wave kernel)");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = dense_reserve(c))) return rc;
    if ((rc = launch_eval_dense(c, true))) return rc;          // fresh f_k(x) into the tracked values; max violation into d_mv
    if (phase == 2 && slack)
        HIPCHK(c, hipMemcpyAsync(c->d_mv, slack, (size_t)c->R * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_sweeps1, 0, (size_t)c->Rpad * sizeof(int64_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_status1, 0, (size_t)c->Rpad * sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_flag, 1, (size_t)c->Rpad, c->stream));
    rc = phase == 1 ? dense_phase<1>(c, 1, viol_tol, tol, seed, first_index, sweep, (int)block, coord_lo, coord_hi)
                    : dense_phase<2>(c, 1, viol_tol, tol, seed, first_index, sweep, (int)block, coord_lo, coord_hi);
    if (rc) return rc;
    HIPCHK(c, spin_sync(c->stream));
    c->evaluated = false;
    return 0;
}

}  // namespace

namespace qcqpmi {

int cd_run_dense(qcqpmi_ctx *c, int phase1, int64_t num_iters, double viol_tol, double tol, uint64_t seed,
                 uint64_t first_index, int64_t *sweeps1, int64_t *sweeps2, int64_t *visits2, int64_t *accepted2,
                 uint8_t *ran_phase2, double *f0, double *maxviol) {
    if (num_iters < 0 || !(tol > 0.0)) return fail(c, QCQPMI_EINVAL, "cd_run: bad num_iters / tol");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = dense_reserve(c))) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_sweeps1, 0, (size_t)c->Rpad * sizeof(int64_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_status1, 0, (size_t)c->Rpad * sizeof(int), c->stream));
    if (phase1) {
        if ((rc = launch_eval_dense(c, true))) return rc;
        if ((rc = dense_phase<1>(c, num_iters, viol_tol, tol, seed, first_index))) return rc;
    }
    if ((rc = launch_eval_dense(c, true))) return rc;   // fresh f_k(x): the slack of phase 2 (qcqp.py:157,189)
    launch_gate(c, viol_tol);
    HIPCHK(c, hipGetLastError());
    if (ran_phase2) HIPCHK(c, hipMemcpyAsync(ran_phase2, c->d_flag, (size_t)c->R, hipMemcpyDeviceToHost, c->stream));
    if ((rc = dense_phase<2>(c, num_iters, viol_tol, tol, seed, first_index))) return rc;
    // (objective, max violation) of the final points: the tracked function values (no third pass over all matrices)
    hipLaunchKernelGGL(dense_tracked_out_kernel, dim3((unsigned)((c->R + 255) / 256)), dim3(256), 0, c->stream, (const double *)c->dn_Ft,
                       c->dn_relop, (int)(c->m + 1), (int)((c->m + 1 + 63) / 64 * 64), c->R, c->d_f0, c->d_mv);
    HIPCHK(c, hipGetLastError());
    c->evaluated = true;
    std::vector<int> st, st1;
    if ((rc = fetch_cd_outputs(c, sweeps1, sweeps2, visits2, accepted2, nullptr, f0, maxviol, st, st1))) return rc;
    if ((rc = cd_apply_status(c, st, st1, f0, maxviol, DN_SC))) return rc;
    return 0;
}

}  // namespace qcqpmi

// ============================================================================================

extern "C" {

int qcqpmi_set_quad_generated(qcqpmi_ctx *c, int64_t k, uint64_t seed, double scale, double qscale,
                              double diag_add, double r, int relop) {
    if (!c) return QCQPMI_EINVAL;
    if (c->finalized) return fail(c, QCQPMI_ESTATE, "set_quad_generated after finalize");
    if (k < 0 || k > c->m) return fail(c, QCQPMI_EINVAL, "set_quad_generated: bad k");
    if ((k == 0) != (relop == 0) || relop < 0 || relop > 2)
        return fail(c, QCQPMI_EINVAL, "set_quad_generated: relop %d invalid for function %lld", relop, (long long)k);
    HostQuad &h = c->quads[(size_t)k];
    h = HostQuad();
    h.gen = true; h.gseed = seed; h.gscale = scale; h.gqscale = qscale; h.gdiag = diag_add;
    h.r = r; h.relop = relop; h.set = true;
    // the linear term comes back to the host (n values): the generic finalize code reads it there
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<double> dq;
    HIPCHK(c, dq.reserve(c->stream, (size_t)c->n, false));
    hipLaunchKernelGGL(dense_gen_q_kernel, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream, dq.p, c->n, (int)k, seed, qscale);
    h.q.resize((size_t)c->n);
    HIPCHK(c, hipMemcpyAsync(h.q.data(), dq.p, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

int qcqpmi_pop_weighted_product(qcqpmi_ctx *c, const double *w, double *Y) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!w || !Y) return fail(c, QCQPMI_EINVAL, "pop_weighted_product: w / Y missing");
    HIPCHK(c, hipSetDevice(c->device));
    DenseProblem D = dense_problem(c);
    if (!c->dn_Gpack) {
        // separable constraints: only the objective has a matrix (the packed P0 of the separable path: the same fragment
        // layout with one function); the weights of the constraints are the caller's business (elementwise operators)
        D.Gpack = c->dp.Apack; D.m1 = 1; D.m1p = 64; D.q = nullptr; D.qT = nullptr; D.r = nullptr; D.relop = nullptr;
    }
    const int64_t n16 = c->n16;
    HIPCHK(c, c->d_ww.reserve(c->stream, (size_t)D.m1, false));
    HIPCHK(c, c->d_wS.reserve(c->stream, (size_t)n16 * n16, false));
    HIPCHK(c, c->d_wz.reserve(c->stream, (size_t)n16));   // zero offset vector of the affine map
    HIPCHK(c, c->d_wY.reserve(c->stream, (size_t)c->Rpad * n16, false));
    double *dw = c->d_ww, *dS = c->d_wS, *dY = c->d_wY, *dz = c->d_wz;
    const int64_t total = c->R * c->n;
    if ((rc = pin_reserve(c, (size_t)total * sizeof(double) + (size_t)D.m1 * sizeof(double)))) return rc;
    char *hw = c->h_pin + (size_t)total * sizeof(double);       // the weights go up through pinned memory too
    memcpy(hw, w, (size_t)D.m1 * sizeof(double));
    HIPCHK(c, hipMemcpyAsync(dw, hw, (size_t)D.m1 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(dense_wsum_pack_kernel, dim3((unsigned)((n16 * n16 + 255) / 256)), dim3(256), 0, c->stream, D, (const double *)dw, dS);
    if ((rc = launch_dense_product(c, 3, dS, dz, c->X, dY))) return rc;
    launch_from_tiles(c, dY, c->R);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_pin, c->d_stage, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    memcpy(Y, c->h_pin, (size_t)total * sizeof(double));
    return 0;
}

int qcqpmi_weighted_matrix(qcqpmi_ctx *c, const double *w, double *S) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!w || !S) return fail(c, QCQPMI_EINVAL, "weighted_matrix: w / S missing");
    if (!c->dn_Gpack) return fail(c, QCQPMI_EUNSUPPORTED, "weighted_matrix needs the packed dense matrices");
    HIPCHK(c, hipSetDevice(c->device));
    const DenseProblem D = dense_problem(c);
    const int64_t n = c->n, n16 = c->n16;
    DevBuf<double> dw, dS, dU;
    HIPCHK(c, dw.reserve(c->stream, (size_t)D.m1, false));
    HIPCHK(c, dS.reserve(c->stream, (size_t)n16 * n16, false));
    HIPCHK(c, dU.reserve(c->stream, (size_t)n * n, false));
    HIPCHK(c, hipMemcpyAsync(dw.p, w, (size_t)D.m1 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(dense_wsum_pack_kernel, dim3((unsigned)((n16 * n16 + 255) / 256)), dim3(256), 0, c->stream, D, (const double *)dw.p, dS.p);
    hipLaunchKernelGGL(dense_unpack_kernel, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, c->stream, (const double *)dS.p, dU.p, n, (int)(n16 / 4));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(S, dU.p, (size_t)n * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

int qcqpmi_pop_eval_parts(qcqpmi_ctx *c, double *quad, double *lin) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!quad || !lin) return fail(c, QCQPMI_EINVAL, "pop_eval_parts: outputs missing");
    if (!c->dn_Gpack) return fail(c, QCQPMI_EUNSUPPORTED, "pop_eval_parts needs the packed dense matrices (constraints that couple coordinates)");
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = eval_parts_dense(c))) return rc;
    const int64_t m1 = c->m + 1;
    const double *dlin = c->d_F + (int64_t)c->eval_zs * m1 * c->Rpad;
    // the two planes ([m1][Rpad], contiguous) through pinned memory in one copy each, the padding columns dropped on the host
    const size_t plane = (size_t)m1 * c->Rpad * sizeof(double);
    if ((rc = pin_reserve(c, 2 * plane))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->h_pin, c->d_F, plane, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_pin + plane, dlin, plane, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    const double *hq = (const double *)c->h_pin.p, *hl = (const double *)(c->h_pin + plane);
    for (int64_t k = 0; k < m1; k++) {
        memcpy(quad + k * c->R, hq + k * c->Rpad, (size_t)c->R * sizeof(double));
        memcpy(lin + k * c->R, hl + k * c->Rpad, (size_t)c->R * sizeof(double));
    }
    c->evaluated = false;    // plane 0 no longer holds the full function values
    return 0;
}

int qcqpmi_cd_dense_block_step(qcqpmi_ctx *c, int phase, int64_t sweep, int64_t block, int coord_lo, int coord_hi, double viol_tol,
                               double tol, uint64_t seed, uint64_t first_index, const double *slack) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!dense_on(c)) return fail(c, QCQPMI_EUNSUPPORTED, "cd_dense_block_step: the problem does not take the dense-constraint path");
    c->last_cd2_kernel = dense_chain_name(c);
    return cd_dense_block_step(c, phase, sweep, block, coord_lo, coord_hi, viol_tol, tol, seed, first_index, slack);
}

int qcqpmi_dense_chain_geometry(int64_t m, int *out4) {
    if (m < 0 || m > (1 << 24) || !out4) return QCQPMI_EINVAL;
    const MwGeom g = mw_geometry((int)m + 1);
    out4[0] = g.SL; out4[1] = g.Tc; out4[2] = g.ts; out4[3] = g.T;
    return 0;
}

int qcqpmi_dense_chain_mode(qcqpmi_ctx *c, int mode) {
    if (!c || mode < 0 || mode > 1) return QCQPMI_EINVAL;
    c->dense_chain_mode = mode;
    return 0;
}

int qcqpmi_debug_dense_profile(qcqpmi_ctx *c, int64_t *out64) {
    if (!c || !out64) return QCQPMI_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    return dense_profile_read(c, out64);
}

}  // extern "C"
