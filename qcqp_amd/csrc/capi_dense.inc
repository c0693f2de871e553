// Host side of the dense-constraint path (cd_dense.h): packing at finalize, MFMA evaluation of all
// m+1 functions, and the sweep / block loops of coordinate descent.  Included by capi.hip.

namespace {

bool dense_on(const qcqpmi_ctx *c) { return !c->sep && c->dn_Gpack && (c->n > 64 || c->dn_force || (c->dbg & 32)); }

DenseProblem dense_problem(const qcqpmi_ctx *c) {
    DenseProblem D;
    D.Gpack = c->dn_Gpack; D.q = c->dn_q; D.r = c->dn_r; D.relop = c->dn_relop;
    D.qT = c->dn_qT;
    D.n = c->n; D.n16 = c->n16; D.NB = (int)(c->n16 / 16); D.KS = (int)(c->n16 / 4); D.m1 = (int)c->m + 1;
    D.m1p = (D.m1 + 63) / 64 * 64;
    return D;
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
            hipLaunchKernelGGL(dense_pack_kernel, dim3(pb, 1), dim3(256), 0, c->stream, (const double *)nullptr,
                               (const double *)(c->dn_tmp - (k - 1) * n * n), gp, n, n16, (int)m1, (int)k);
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

int ensure_F(qcqpmi_ctx *c) {
    HIPCHK(c, c->d_F.reserve(c->stream, (size_t)((c->m + 1) * c->Rpad)));
    return 0;
}

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

}  // namespace

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
    hipLaunchKernelGGL(gate_kernel, dim3((unsigned)((c->Rpad + 255) / 256)), dim3(256), 0, c->stream, c->d_mv,
                       c->d_status1, c->d_flag, c->R, c->Rpad, viol_tol);
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
