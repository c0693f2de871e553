// ADMM part of the C ABI: setup (qcqpmi_admm_set_eig / set_basis / setup / zsolver_device),
// the unit operator qcqpmi_admm_onecons and the iteration qcqpmi_admm_run.  Every product of the iteration goes through
// the engine's own fp64 GEMM (gemm_pk.h); the algorithm itself is in admm.h.  rocSOLVER -- and the rocBLAS handle it
// wants -- is loaded lazily for the optional device-side eigendecompositions of qcqpmi_admm_setup only.
// The one unit that compiles the kernels of admm.h and gemm_pk.h.
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "capi_ctx.h"
#include "admm.h"
#include "admm_fused.h"
#include "gemm_pk.h"

using namespace qcqpmi;

namespace {

struct RocblasApi {
    void *h = nullptr;
    int (*create)(void **) = nullptr;
    int (*destroy)(void *) = nullptr;
    int (*set_stream)(void *, hipStream_t) = nullptr;
};

RocblasApi *rocblas() {
    static RocblasApi api;
    static bool tried = false;
    if (!tried) {
        tried = true;
        const char *names[] = {"librocblas.so", "librocblas.so.5", "/opt/rocm/lib/librocblas.so"};
        for (const char *nm : names) {
            api.h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
            if (api.h) break;
        }
        if (api.h) {
            api.create = (decltype(api.create))dlsym(api.h, "rocblas_create_handle");
            api.destroy = (decltype(api.destroy))dlsym(api.h, "rocblas_destroy_handle");
            api.set_stream = (decltype(api.set_stream))dlsym(api.h, "rocblas_set_stream");
        }
    }
    return (api.h && api.create && api.set_stream) ? &api : nullptr;
}

// rocSOLVER (batched symmetric eigensolver for the device-side ADMM setup), loaded lazily like rocBLAS
struct RocsolverApi {
    void *h = nullptr;
    int (*dsyevd_sb)(void *, int, int, int, double *, int, int64_t, double *, int64_t, double *, int64_t, int *, int) = nullptr;
};

RocsolverApi *rocsolver() {
    static RocsolverApi api;
    static bool tried = false;
    if (!tried) {
        tried = true;
        const char *names[] = {"librocsolver.so", "librocsolver.so.0", "/opt/rocm/lib/librocsolver.so"};
        for (const char *nm : names) {
            api.h = dlopen(nm, RTLD_LAZY | RTLD_GLOBAL);
            if (api.h) break;
        }
        if (api.h) api.dsyevd_sb = (decltype(api.dsyevd_sb))dlsym(api.h, "rocsolver_dsyevd_strided_batched");
    }
    return (api.h && api.dsyevd_sb) ? &api : nullptr;
}

// qhat_k = Q_k^T q_k and the multiplier bracket (-1/lambda over the positive / negative eigenvalues,
// utilities.py:166,176-180) from the device-resident eigenpairs: one workgroup per constraint
__global__ __launch_bounds__(256) void admm_setup_finish_kernel(const double *__restrict__ W, const double *__restrict__ lam,
                                                                const double *__restrict__ gq, int64_t n, int64_t n16,
                                                                double *__restrict__ qhat, double *__restrict__ slo,
                                                                double *__restrict__ ehi) {
    __shared__ double rs[256], re[256];
    const int64_t k = blockIdx.x;
    const double *Wk = W + k * n * n, *q = gq + k * n16;
    double s = -INFINITY, e = INFINITY;
    for (int64_t j = threadIdx.x; j < n; j += 256) {
        const double *col = Wk + j * n;     // eigenvector j (column-major block)
        double acc = 0.0;
        for (int64_t i = 0; i < n; i++) acc += col[i] * q[i];
        qhat[k * n + j] = acc;
        const double l = lam[k * n + j];
        if (l > 0.0) { const double v = -1.0 / l; s = v > s ? v : s; }
        if (l < 0.0) { const double v = -1.0 / l; e = v < e ? v : e; }
    }
    rs[threadIdx.x] = s; re[threadIdx.x] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < 256; t++) { s = rs[t] > s ? rs[t] : s; e = re[t] < e ? re[t] : e; }
        slo[k] = s; ehi[k] = e;
    }
}

__global__ void admm_symmetrise_kernel(double *__restrict__ A, int64_t n, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int64_t k = idx / (n * n), rem = idx % (n * n), i = rem / n, j = rem % n;
    if (i < j) {
        double *M = A + k * n * n;
        const double v = 0.5 * (M[i * n + j] + M[j * n + i]);   // (P + P^T) / 2 like the reference's eigh input
        M[i * n + j] = v; M[j * n + i] = v;
    }
}

#define RBCHK(c, expr)                                                              \
    do {                                                                            \
        int s_ = (expr);                                                            \
        if (s_ != 0) return fail(c, QCQPMI_EHIP, "%s failed: rocblas status %d", #expr, s_); \
    } while (0)

}  // namespace

void qcqpmi::admm_drop_handle(qcqpmi_ctx *c) {
    if (c->rb_handle && rocblas() && rocblas()->destroy) rocblas()->destroy(c->rb_handle);
    c->rb_handle = nullptr;
}

namespace {

// drops the installed basis; ad_Minvpk stays: a new basis does not invalidate (2 (P0 + rho m I))^-1
void admm_free(qcqpmi_ctx *c) {
    c->ad_WTpk.release(); c->ad_Wpk.release(); c->ad_lam.release(); c->ad_qhat.release(); c->ad_rk.release(); c->ad_relop.release();
    c->ad_slo.release(); c->ad_ehi.release(); c->ad_uidx.release(); c->ad_uptr.release(); c->ad_ulist.release(); c->ad_usgn.release();
    c->ad_unit = false;
    c->ad_rows = 0; c->ad_Mh16 = 0; c->ad_lowrank = 0;
    admm_drop_handle(c);
}

int gemm_pk(qcqpmi_ctx *c, const double *A, const double *B, double *C, const double *bias, int MB, int KB, int ntiles, int zs,
            double alpha = 1.0) {
    GemmPkArgs g;
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.MB = MB; g.KB = KB; g.ntiles = ntiles; g.zs = zs; g.alpha = alpha;
    const int64_t wg_big = (int64_t)((MB + GP_FG - 1) / GP_FG) * ((ntiles + GP_TG - 1) / GP_TG) * zs;
    if (wg_big < 256) {     // fewer workgroups than CUs: 64 x 64 output tiles (same arithmetic, same summation order per output)
        hipLaunchKernelGGL(gemm_pk_small_kernel, dim3((unsigned)((MB + GS_FG - 1) / GS_FG), (unsigned)((ntiles + GS_TG - 1) / GS_TG), (unsigned)zs),
                           dim3(256), GS_LDS_BYTES, c->stream, g);
    } else {
        hipLaunchKernelGGL(gemm_pk_kernel, dim3((unsigned)((MB + GP_FG - 1) / GP_FG), (unsigned)((ntiles + GP_TG - 1) / GP_TG), (unsigned)zs),
                           dim3(256), GP_LDS_BYTES, c->stream, g);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

// grid.z of a product with few outputs and a long contraction: enough workgroups for two per CU, at most 16 planes
int gemm_zsplit(int MB, int ntiles, int KB) {
    const int64_t wg = (int64_t)((MB + GP_FG - 1) / GP_FG) * ((ntiles + GP_TG - 1) / GP_TG);
    int zs = (int)((512 + wg - 1) / wg);
    zs = std::min(std::min(zs, 16), KB / 8);      // a plane needs a contraction worth a launch (>= 8 k-blocks = 128 columns):
    return std::max(zs, 1);                       // summing planes costs a pass over the output per plane
}

// Wd: [m][rows][n] on the device (basis vector j of constraint k contiguous) -> the two packed operators
//   WTpk  rows h = k rows + j, columns i   (ZQ = W^T Z)       Wpk  rows i, columns h   (S = W D)
int admm_install_basis(qcqpmi_ctx *c, const double *Wd, int64_t rows) {
    const int64_t n = c->n, n16 = c->n16, m = c->m;
    const int64_t Mh = m * rows, Mh16 = (Mh + 15) / 16 * 16;
    if (Mh16 / 16 > 2147483647LL / 64 || Mh16 * n16 > (int64_t)1 << 40) return fail(c, QCQPMI_EUNSUPPORTED, "admm: basis too large");
    HIPCHK(c, c->ad_WTpk.reserve(c->stream, (size_t)Mh16 * n16, false));
    HIPCHK(c, c->ad_Wpk.reserve(c->stream, (size_t)Mh16 * n16, false));
    const int MBh = (int)(Mh16 / 16), KBn = (int)(n16 / 16);
    const int64_t tot = Mh16 * n16;
    hipLaunchKernelGGL(gemm_pk_pack_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, Wd, c->ad_WTpk, Mh, n, n, (int64_t)1, MBh, KBn);
    hipLaunchKernelGGL(gemm_pk_pack_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, Wd, c->ad_Wpk, n, Mh, (int64_t)1, n, KBn, MBh);
    HIPCHK(c, hipGetLastError());
    c->ad_rows = rows; c->ad_Mh16 = Mh16;
    return 0;
}

// host side of both set_eig and set_basis: bracket of the multiplier from the nonzero eigenvalues (utilities.py:176-180)
void admm_brackets(const double *lam, int64_t m, int64_t rows, std::vector<double> &slo, std::vector<double> &ehi) {
    slo.assign((size_t)m, -INFINITY); ehi.assign((size_t)m, INFINITY);
    for (int64_t k = 0; k < m; k++)
        for (int64_t j = 0; j < rows; j++) {
            const double l = lam[k * rows + j];
            if (l > 0.0) { const double v = -1.0 / l; if (v > slo[(size_t)k]) slo[(size_t)k] = v; }
            if (l < 0.0) { const double v = -1.0 / l; if (v < ehi[(size_t)k]) ehi[(size_t)k] = v; }
        }
}

int admm_upload_small(qcqpmi_ctx *c, const double *lam, const double *qhat, int64_t rows) {
    const int64_t m = c->m;
    std::vector<double> rk((size_t)m), slo, ehi;
    std::vector<int> relop((size_t)m);
    for (int64_t k = 0; k < m; k++) { rk[(size_t)k] = c->quads[(size_t)k + 1].r; relop[(size_t)k] = c->quads[(size_t)k + 1].relop; }
    admm_brackets(lam, m, rows, slo, ehi);
    c->ad_qzero = true;
    for (int64_t t = 0; t < m * rows; t++) if (qhat[t] != 0.0) { c->ad_qzero = false; break; }
    int rc;
    auto up = [&](DevBuf<double> &dst, const double *src, size_t cnt) -> int {
        HIPCHK(c, dst.reserve(c->stream, cnt, false));
        HIPCHK(c, hipMemcpyAsync(dst.p, src, cnt * sizeof(double), hipMemcpyHostToDevice, c->stream));
        return 0;
    };
    if ((rc = up(c->ad_lam, lam, (size_t)m * rows))) return rc;
    if ((rc = up(c->ad_qhat, qhat, (size_t)m * rows))) return rc;
    if ((rc = up(c->ad_rk, rk.data(), rk.size()))) return rc;
    if ((rc = up(c->ad_slo, slo.data(), slo.size()))) return rc;
    if ((rc = up(c->ad_ehi, ehi.data(), ehi.size()))) return rc;
    HIPCHK(c, c->ad_relop.reserve(c->stream, (size_t)m, false));
    HIPCHK(c, hipMemcpyAsync(c->ad_relop, relop.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

void admm_fill_args(qcqpmi_ctx *c, AdmmArgs &sa, int64_t R) {
    sa.n = c->n; sa.m = c->m; sa.R = R; sa.rows_k = c->ad_rows; sa.Mh16 = c->ad_Mh16;
    sa.lam = c->ad_lam; sa.qhat = c->ad_qhat; sa.rk = c->ad_rk; sa.relop = c->ad_relop; sa.slo = c->ad_slo; sa.ehi = c->ad_ehi;
    sa.first_iter = 0; sa.viol_only = 0; sa.lowrank = c->ad_lowrank; sa.project_only = 0; sa.sec_tol = 1e-6;
    sa.zq_planes = 1; sa.zq_plane = 0;
    sa.no_shortcut = (c->dbg & 8) ? 1 : 0;
}

int admm_launch_secular(qcqpmi_ctx *c, const AdmmArgs &sa) {
    hipStream_t st = c->stream;
    const int64_t rows = sa.rows_k, Rp = (sa.R + 15) / 16 * 16;
    tic(c, 4);
    if (sa.lowrank && rows <= 8) {
        const unsigned g = (unsigned)((sa.m * Rp + 255) / 256);
        if (rows == 1) hipLaunchKernelGGL(admm_secular_small_kernel<1>, dim3(g), dim3(256), 0, st, sa);       // (the template argument IS the row stride)
        else if (rows == 2) hipLaunchKernelGGL(admm_secular_small_kernel<2>, dim3(g), dim3(256), 0, st, sa);
        else if (rows == 4) hipLaunchKernelGGL(admm_secular_small_kernel<4>, dim3(g), dim3(256), 0, st, sa);
        else if (rows == 8) hipLaunchKernelGGL(admm_secular_small_kernel<8>, dim3(g), dim3(256), 0, st, sa);
        else return fail(c, QCQPMI_EUNSUPPORTED, "admm: reduced bases come with 1, 2, 4 or 8 rows per constraint (pad with zero rows), or more than 8");
    } else {
        const unsigned g = (unsigned)((sa.m * Rp + 3) / 4);
        AdmmArgs s2 = sa;
        s2.R = sa.R;
        // (elements per lane: slots past rows_k only add exact zeros to the sums -- the instantiations give identical bits)
        if (rows <= 128) hipLaunchKernelGGL(admm_secular_kernel<2>, dim3(g), dim3(256), 0, st, s2);
        else if (rows <= 256) hipLaunchKernelGGL(admm_secular_kernel<4>, dim3(g), dim3(256), 0, st, s2);
        else if (rows <= 512) hipLaunchKernelGGL(admm_secular_kernel<8>, dim3(g), dim3(256), 0, st, s2);
        else if (rows <= 1024) hipLaunchKernelGGL(admm_secular_kernel<16>, dim3(g), dim3(256), 0, st, s2);
        else if (rows <= 2048) hipLaunchKernelGGL(admm_secular_kernel<32>, dim3(g), dim3(256), 0, st, s2);
        else if (rows <= 4096) hipLaunchKernelGGL(admm_secular_kernel<64>, dim3(g), dim3(256), 0, st, s2);
        else {
            // more than 4096 hat rows per constraint (full eigenbasis at n > 4096): a workgroup per (constraint, restart) pair
            const unsigned gw = (unsigned)(sa.m * Rp);
            if (rows <= 8192) hipLaunchKernelGGL((admm_secular_kernel<32, 4>), dim3(gw), dim3(256), 0, st, s2);
            else hipLaunchKernelGGL((admm_secular_kernel<64, 4>), dim3(gw), dim3(256), 0, st, s2);
        }
    }
    toc(c, 4);
    HIPCHK(c, hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int qcqpmi_admm_set_eig(qcqpmi_ctx *c, const double *lmb, const double *Q) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!lmb || !Q) return fail(c, QCQPMI_EINVAL, "admm_set_eig: lmb / Q missing");
    if (c->m < 1) return fail(c, QCQPMI_EINVAL, "admm needs at least one constraint");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->n, m = c->m;
    admm_free(c);
    // Wd[k][j][i] = Q_k[i][j]: eigenvector j of constraint k contiguous (NumPy's eigh layout transposed)
    std::vector<double> W((size_t)m * n * n), qhat((size_t)m * n);
    for (int64_t k = 0; k < m; k++) {
        const double *Qk = Q + k * n * n;
        double *Wk = W.data() + k * n * n;
        for (int64_t i = 0; i < n; i++)
            for (int64_t j = 0; j < n; j++) Wk[j * n + i] = Qk[i * n + j];
        const HostQuad &h = c->quads[(size_t)k + 1];
        for (int64_t j = 0; j < n; j++) {   // qhat = Q^T q  (utilities.py:166)
            double acc = 0.0;
            for (int64_t i = 0; i < n; i++) acc += Qk[i * n + j] * h.q[(size_t)i];
            qhat[(size_t)(k * n + j)] = acc;
        }
    }
    DevBuf<double> Wd;
    HIPCHK(c, Wd.reserve(c->stream, W.size(), false));
    HIPCHK(c, hipMemcpyAsync(Wd.p, W.data(), W.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = admm_install_basis(c, Wd.p, n))) return rc;
    if ((rc = admm_upload_small(c, lmb, qhat.data(), n))) return rc;
    c->ad_lowrank = 0;
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

// ---- unit bases.  When every basis vector is +-e_i (separable constraints p x_i^2 + q x_i + r ~ 0: Boolean least squares,
// MAXCUT, boxes -- the eigenvectors utilities.py:160-162 gets from LAPACK for a diagonal matrix are unit vectors) the two consensus
// products of an iteration move single entries: ZQ[h] = s_h Z[i_h] and S[i] = sum over the rows h on coordinate i of s_h D[h], the
// values the GEMMs produce (a sum of one term and zeros), without reading an n x (m rp) operator twice per iteration.
__global__ void admm_unit_gather_kernel(const double *__restrict__ Z, double *__restrict__ ZQ, const int *__restrict__ uidx,
                                        const double *__restrict__ usgn, int64_t n16, int64_t Mh16, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // element (tile, row h, column)
    if (e >= total) return;
    const int64_t col = e & 15, h = (e >> 4) % Mh16, t = (e >> 4) / Mh16;
    const int i = uidx[h];
    ZQ[e] = i >= 0 ? usgn[h] * Z[(t * n16 + i) * 16 + col] : 0.0;
}
__global__ void admm_unit_scatter_kernel(const double *__restrict__ D, double *__restrict__ S, const int *__restrict__ uptr,
                                         const int *__restrict__ ulist, const double *__restrict__ usgn, int64_t n16, int64_t Mh16, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // element (tile, coordinate, column)
    if (e >= total) return;
    const int64_t col = e & 15, i = (e >> 4) % n16, t = (e >> 4) / n16;
    double s = 0.0;
    for (int k = uptr[i]; k < uptr[i + 1]; k++) { const int h = ulist[k]; s += usgn[h] * D[(t * Mh16 + h) * 16 + col]; }
    S[e] = s;
}

// does the basis consist of unit vectors?  (host copy Bv: [m][rows][n]) -> index / sign / CSR tables on the device
int admm_install_unit(qcqpmi_ctx *c, const double *Bv, int64_t rows) {
    const int64_t n = c->n, n16 = c->n16, m = c->m, Mh = m * rows, Mh16 = (Mh + 15) / 16 * 16;
    std::vector<int> idx((size_t)Mh16, -1);
    std::vector<double> sgn((size_t)Mh16, 0.0);
    for (int64_t h = 0; h < Mh; h++) {
        const double *v = Bv + h * n;
        int64_t at = -1;
        for (int64_t j = 0; j < n; j++) {
            if (v[j] == 0.0) continue;
            if (at >= 0 || (v[j] != 1.0 && v[j] != -1.0)) return 0;       // not a unit basis: the GEMM path
            at = j;
        }
        if (at < 0) return 0;
        idx[(size_t)h] = (int)at; sgn[(size_t)h] = v[at];
    }
    std::vector<int> ptr((size_t)n16 + 1, 0), list((size_t)std::max<int64_t>(Mh, 1));
    for (int64_t h = 0; h < Mh; h++) ptr[(size_t)idx[(size_t)h] + 1]++;
    for (int64_t i = 0; i < n16; i++) ptr[(size_t)i + 1] += ptr[(size_t)i];
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    for (int64_t h = 0; h < Mh; h++) list[(size_t)fill[(size_t)idx[(size_t)h]]++] = (int)h;     // ascending h per coordinate
    HIPCHK(c, c->ad_uidx.reserve(c->stream, idx.size(), false));
    HIPCHK(c, c->ad_usgn.reserve(c->stream, sgn.size(), false));
    HIPCHK(c, c->ad_uptr.reserve(c->stream, ptr.size(), false));
    HIPCHK(c, c->ad_ulist.reserve(c->stream, list.size(), false));
    HIPCHK(c, hipMemcpyAsync(c->ad_uidx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->ad_usgn, sgn.data(), sgn.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->ad_uptr, ptr.data(), ptr.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->ad_ulist, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    c->ad_unit = true;
    return 0;
}

int qcqpmi_admm_set_basis(qcqpmi_ctx *c, int64_t rp, const double *lam, const double *Bv, const double *qhat) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!lam || !Bv || !qhat || rp < 1 || rp > c->n) return fail(c, QCQPMI_EINVAL, "admm_set_basis: bad arguments");
    if (c->m < 1) return fail(c, QCQPMI_EINVAL, "admm needs at least one constraint");
    // the small secular kernels and the fused kernel are instantiated for 1, 2, 4, 8 rows (the template argument is the row
    // stride); refused HERE, before anything is uploaded, not at the first qcqpmi_admm_run (lowrank.py pads with zero rows)
    if (rp == 3 || (rp > 4 && rp < 8))
        return fail(c, QCQPMI_EUNSUPPORTED, "admm_set_basis: reduced bases come with 1, 2, 4 or 8 rows per constraint (pad with zero rows), or more than 8");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->n, m = c->m;
    admm_free(c);
    DevBuf<double> Wd;
    HIPCHK(c, Wd.reserve(c->stream, (size_t)m * rp * n, false));
    HIPCHK(c, hipMemcpyAsync(Wd.p, Bv, (size_t)m * rp * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = admm_install_basis(c, Wd.p, rp))) return rc;
    if ((rc = admm_upload_small(c, lam, qhat, rp))) return rc;
    if ((rc = admm_install_unit(c, Bv, rp))) return rc;
    c->ad_lowrank = 1;
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

int qcqpmi_admm_set_bracket(qcqpmi_ctx *c, const double *slo, const double *ehi) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!slo || !ehi) return fail(c, QCQPMI_EINVAL, "admm_set_bracket: bad arguments");
    if (!c->ad_slo || !c->ad_ehi) return fail(c, QCQPMI_ESTATE, "admm_set_bracket: no eigenpairs / bases installed");
    for (int64_t k = 0; k < c->m; k++)
        if (!(slo[k] <= 0.0) || !(ehi[k] >= 0.0)) return fail(c, QCQPMI_EINVAL, "admm_set_bracket: constraint %lld: need slo <= 0 <= ehi", (long long)(k + 1));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->ad_slo, slo, (size_t)c->m * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->ad_ehi, ehi, (size_t)c->m * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

int qcqpmi_admm_apply_constraints(qcqpmi_ctx *c, int p, const double *Vin, int shared, double *out) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!Vin || !out || p < 1 || p > 64) return fail(c, QCQPMI_EINVAL, "admm_apply_constraints: bad arguments");
    if (!c->d_gP) return fail(c, QCQPMI_EUNSUPPORTED, "admm_apply_constraints: needs the dense constraint matrices on the device "
                                                        "(constraints that couple coordinates, given with qcqpmi_set_quad)");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->n, m = c->m;
    DevBuf<double> dV, dO;
    const size_t vin = (size_t)(shared ? 1 : m) * n * p, vout = (size_t)m * n * p;
    HIPCHK(c, dV.reserve(c->stream, vin, false));
    HIPCHK(c, dO.reserve(c->stream, vout, false));
    HIPCHK(c, hipMemcpyAsync(dV.p, Vin, vin * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(admm_apply_constraints_kernel, dim3((unsigned)((n + 15) / 16), (unsigned)m), dim3(256), 0, c->stream,
                       (const double *)c->d_gP, (const double *)dV.p, dO.p, n, p, shared ? 1 : 0);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, dO.p, vout * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

int qcqpmi_admm_setup(qcqpmi_ctx *c) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (c->m < 1) return fail(c, QCQPMI_EINVAL, "admm needs at least one constraint");
    if (!c->d_gP) return fail(c, QCQPMI_EUNSUPPORTED, "admm_setup: needs the dense constraint matrices on the device "
                                                        "(coupled constraints given with qcqpmi_set_quad); use qcqpmi_admm_set_eig");
    RocblasApi *rb = rocblas();
    RocsolverApi *rsv = rocsolver();
    if (!rb || !rsv) return fail(c, QCQPMI_EHIP, "librocblas.so / librocsolver.so could not be loaded");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->n, m = c->m;
    if (n > 32768 || m > 1000000) return fail(c, QCQPMI_EUNSUPPORTED, "admm_setup: sizes exceed rocSOLVER int range");
    admm_free(c);
    RBCHK(c, rb->create(&c->rb_handle));      // rocSOLVER takes a rocBLAS handle (setup only; no product of the iteration uses it)
    RBCHK(c, rb->set_stream(c->rb_handle, c->stream));
    DevBuf<double> W, E, lam, qh;
    DevBuf<int> info;
    HIPCHK(c, W.reserve(c->stream, (size_t)m * n * n, false));
    HIPCHK(c, lam.reserve(c->stream, (size_t)m * n, false));
    HIPCHK(c, qh.reserve(c->stream, (size_t)m * n, false));
    HIPCHK(c, E.reserve(c->stream, (size_t)m * n, false));
    HIPCHK(c, info.reserve(c->stream, (size_t)m));
    DevBuf<double> slo, ehi;
    HIPCHK(c, slo.reserve(c->stream, (size_t)m, false));
    HIPCHK(c, ehi.reserve(c->stream, (size_t)m, false));
    // symmetric row-major == column-major: the matrices go into W in place and come back as eigenvectors
    HIPCHK(c, hipMemcpyAsync(W.p, c->d_gP, (size_t)m * n * n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    const int64_t tot = m * n * n;
    hipLaunchKernelGGL(admm_symmetrise_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, W.p, n, tot);
    RBCHK(c, rsv->dsyevd_sb(c->rb_handle, 211 /* evect_original */, 121 /* fill_upper */, (int)n, W.p, (int)n, n * n,
                            lam.p, n, E.p, n, info.p, (int)m));
    hipLaunchKernelGGL(admm_setup_finish_kernel, dim3((unsigned)m), dim3(256), 0, c->stream, (const double *)W.p,
                       (const double *)lam.p, c->dp.gq, n, c->n16, qh.p, slo.p, ehi.p);
    HIPCHK(c, hipGetLastError());
    std::vector<int> hinfo((size_t)m);
    std::vector<double> hlam((size_t)m * n), hqh((size_t)m * n);
    HIPCHK(c, hipMemcpyAsync(hinfo.data(), info.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hlam.data(), lam.p, hlam.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hqh.data(), qh.p, hqh.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    for (int64_t k = 0; k < m; k++)
        if (hinfo[(size_t)k] != 0) return fail(c, QCQPMI_EHIP, "admm_setup: eigensolver did not converge for constraint %lld (info %d)", (long long)k + 1, hinfo[(size_t)k]);
    // rocSOLVER's eigenvector j of constraint k is column j of a column-major matrix: contiguous, the layout install wants
    if ((rc = admm_install_basis(c, W.p, n))) return rc;
    if ((rc = admm_upload_small(c, hlam.data(), hqh.data(), n))) return rc;
    c->ad_lowrank = 0;
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

// onecons_qcqp (utilities.py:149-196) as a unit operator: the projection of every resident point onto constraint k
// (1-based) with the installed eigenpairs / basis; out is R x n like qcqpmi_pop_download.  The population is not changed.
int qcqpmi_admm_onecons(qcqpmi_ctx *c, int64_t k, double *out) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!c->ad_WTpk) return fail(c, QCQPMI_ESTATE, "admm_onecons: no eigenpairs installed (qcqpmi_admm_set_eig / set_basis / setup)");
    if (k < 1 || k > c->m || !out) return fail(c, QCQPMI_EINVAL, "admm_onecons: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n16 = c->n16, R = c->R, Rpad = c->Rpad;
    const int ntiles = (int)(Rpad / 16), KBn = (int)(n16 / 16), MBh = (int)(c->ad_Mh16 / 16);
    DevBuf<double> ZQ, Xo;
    DevBuf<uint8_t> act;
    HIPCHK(c, ZQ.reserve(c->stream, (size_t)c->ad_Mh16 * Rpad));
    HIPCHK(c, Xo.reserve(c->stream, (size_t)n16 * Rpad));
    HIPCHK(c, act.reserve(c->stream, (size_t)Rpad));
    HIPCHK(c, hipMemsetAsync(act.p, 1, (size_t)Rpad, c->stream));
    if ((rc = gemm_pk(c, c->ad_WTpk, c->X, ZQ.p, nullptr, MBh, KBn, ntiles, 1))) return rc;
    if (c->ad_lowrank) {
        // keep B^T z: x = z + B (xhat - B^T z)
        DevBuf<double> ZB;
        HIPCHK(c, ZB.reserve(c->stream, (size_t)c->ad_Mh16 * Rpad, false));
        HIPCHK(c, hipMemcpyAsync(ZB.p, ZQ.p, (size_t)c->ad_Mh16 * Rpad * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        AdmmArgs sa;
        admm_fill_args(c, sa, R);
        sa.ZQ = ZQ.p; sa.UH = ZQ.p; sa.act = act.p; sa.mvbits = nullptr; sa.project_only = 1;
        if ((rc = admm_launch_secular(c, sa))) return rc;
        const int64_t tot = c->ad_Mh16 * Rpad;
        hipLaunchKernelGGL(admm_onecons_mask_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, ZQ.p, (const double *)ZB.p,
                           c->ad_Mh16, c->ad_rows, k - 1, tot, 1);
        if ((rc = gemm_pk(c, c->ad_Wpk, ZQ.p, Xo.p, nullptr, KBn, MBh, ntiles, 1))) return rc;
        const int64_t tz = n16 * Rpad;
        hipLaunchKernelGGL(admm_axpy_kernel, dim3((unsigned)((tz + 255) / 256)), dim3(256), 0, c->stream, Xo.p, (const double *)c->X, tz);
        HIPCHK(c, spin_sync(c->stream));
    } else {
        AdmmArgs sa;
        admm_fill_args(c, sa, R);
        sa.ZQ = ZQ.p; sa.UH = ZQ.p; sa.act = act.p; sa.mvbits = nullptr; sa.project_only = 1;
        if ((rc = admm_launch_secular(c, sa))) return rc;
        const int64_t tot = c->ad_Mh16 * Rpad;
        hipLaunchKernelGGL(admm_onecons_mask_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, ZQ.p, (const double *)nullptr,
                           c->ad_Mh16, c->ad_rows, k - 1, tot, 0);
        if ((rc = gemm_pk(c, c->ad_Wpk, ZQ.p, Xo.p, nullptr, KBn, MBh, ntiles, 1))) return rc;
    }
    HIPCHK(c, hipGetLastError());
    const int64_t total = R * c->n;
    launch_from_tiles(c, Xo.p, R);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->d_stage, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, spin_sync(c->stream));
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// Device-side setup of the z-update for a non-diagonal P0 (qcqp.py:224-227: the reference factorises 2 (P0 + rho m I)
// with SuperLU) and of the rho check (qcqp.py:261-278: lambda_min(P0) from LA.eigh).  No LAPACK: the inverse is a
// Newton-Schulz iteration on the engine's own fp64 MFMA GEMM, lambda_min a Lanczos recurrence with device products.

// M = 2 (P0 + shift I) in tile-major [n16/16][n16][16] (padding: identity) and X0 = I / ||M||_inf (tile-major)
__global__ void zs_build_kernel(const double *__restrict__ P0, int64_t n, int64_t n16, double shift, double *__restrict__ Mtm) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n16 * n16) return;
    const int64_t t = idx / (n16 * 16), rem = idx % (n16 * 16), i = rem / 16, j = 16 * t + (rem & 15);
    double v;
    if (i < n && j < n) v = 2.0 * (P0[i * n16 + j] + (i == j ? shift : 0.0));
    else v = (i == j) ? 1.0 : 0.0;
    Mtm[idx] = v;
}

// row sums of |M| (tile-major): one thread per row
__global__ void zs_rowsum_kernel(const double *__restrict__ Mtm, int64_t n16, double *__restrict__ rs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n16) return;
    double s = 0.0;
    for (int64_t t = 0; t < n16 / 16; t++)
        for (int c = 0; c < 16; c++) s += fabs(Mtm[t * n16 * 16 + i * 16 + c]);
    rs[i] = s;
}

__global__ void zs_scaled_identity_kernel(double *__restrict__ Xtm, int64_t n16, double alpha) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n16 * n16) return;
    const int64_t t = idx / (n16 * 16), rem = idx % (n16 * 16), i = rem / 16, j = 16 * t + (rem & 15);
    Xtm[idx] = (i == j) ? alpha : 0.0;
}

// fragment-packed A operand of a SYMMETRIC matrix held tile-major:  Apk[rb][kk][l] = X[16 rb + (l & 15)][4 kk + (l >> 4)]
//  = X[4 kk + (l >> 4)][16 rb + (l & 15)] = Xtm[rb][4 kk + (l >> 4)][l & 15]
__global__ void zs_pack_sym_kernel(const double *__restrict__ Xtm, double *__restrict__ Apk, int64_t n16) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n16 * n16) return;
    const int l = (int)(idx & 63);
    const int64_t fk = idx >> 6, KS = n16 / 4, rb = fk / KS, kk = fk % KS;
    Apk[idx] = Xtm[rb * n16 * 16 + (4 * kk + (l >> 4)) * 16 + (l & 15)];
}

// X <- 2 X - U  and the residual  max |T - I|  (T = M X of this iteration), block-reduced with atomicMax on the bits
__global__ void zs_update_kernel(double *__restrict__ Xtm, const double *__restrict__ Utm, const double *__restrict__ Ttm,
                                 int64_t n16, unsigned long long *__restrict__ resid_bits) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double r = 0.0;
    if (idx < n16 * n16) {
        const int64_t t = idx / (n16 * 16), rem = idx % (n16 * 16), i = rem / 16, j = 16 * t + (rem & 15);
        Xtm[idx] = 2.0 * Xtm[idx] - Utm[idx];
        r = fabs(Ttm[idx] - (i == j ? 1.0 : 0.0));
    }
    __shared__ double red[256];
    red[threadIdx.x] = r;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(resid_bits, (unsigned long long)__double_as_longlong(red[0]));   // non-negative doubles order like integers
}

// R = I - M X (tile-major) with every product and sum carried in double-double (TwoProduct by fma, TwoSum): the residual of an
// inverse that is already at fp64 rounding level, exact to a few units of 1e-32 -- what the refinement step X <- X + X R needs.
// (An fp64 GEMM cannot give it: its own rounding, ~sqrt(n) eps, is the size of the residual.)  One thread per entry.
__global__ void zs_resid_dd_kernel(const double *__restrict__ Mtm, const double *__restrict__ Xtm, int64_t n16, double *__restrict__ Rtm) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n16 * n16) return;
    const int64_t t = idx / (n16 * 16), rem = idx % (n16 * 16), i = rem / 16, j = 16 * t + (rem & 15);
    double s = (i == j) ? 1.0 : 0.0, e = 0.0;            // s + e = I_ij - sum_k M_ik X_kj
    for (int64_t k = 0; k < n16; k++) {
        const double a = Mtm[(k >> 4) * n16 * 16 + i * 16 + (k & 15)];
        const double b = Xtm[t * n16 * 16 + k * 16 + (j & 15)];
        const double p = -a * b;
        const double pe = fma(-a, b, -p);                 // -a b = p + pe exactly
        const double u = s + p, v = u - s;
        e += ((s - (u - v)) + (p - v)) + pe;              // s + p = u + (TwoSum error)
        s = u;
    }
    Rtm[idx] = s + e;
}

__global__ void zs_add_kernel(double *__restrict__ Xtm, const double *__restrict__ Utm, int64_t tot) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < tot) Xtm[idx] += Utm[idx];
}

// (2 (P0 + rho m I))^-1 on the device, left fragment-packed for the z-update GEMM of qcqpmi_admm_run (Minv = NULL).
//   X_{k+1} = X_k (2 I - M X_k),  X_0 = I / ||M||_inf  (M symmetric positive definite: converges quadratically once
//   ||I - M X|| < 1, about log2(cond M) + 6 iterations), then one refinement step with the residual in double-double.
//   resid_out = (max |I - M X| of the last iteration checked)^2: the estimate for the iterate before the refinement.
int qcqpmi_admm_zsolver_device(qcqpmi_ctx *c, double rho, int64_t max_iter, double *resid_out, int64_t *iters_out) {
    if (!c) return QCQPMI_EINVAL;
    if (!c->finalized) return fail(c, QCQPMI_ESTATE, "admm_zsolver_device: context not finalized");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->n, n16 = c->n16, m = c->m, tot = n16 * n16;
    const int KBn = (int)(n16 / 16), nt = KBn;
    if (max_iter <= 0) max_iter = 80;
    hipStream_t st = c->stream;
    int rc;
    DevBuf<double> Mtm, Mpk, Xtm, Xpk, Ttm, Utm, rs;
    DevBuf<unsigned long long> rb;
    for (DevBuf<double> *b : {&Mtm, &Mpk, &Xtm, &Xpk, &Ttm, &Utm}) HIPCHK(c, b->reserve(st, (size_t)tot, false));
    HIPCHK(c, rs.reserve(st, (size_t)n16, false));
    HIPCHK(c, rb.reserve(st, 1, false));
    const dim3 gb((unsigned)((tot + 255) / 256)), tb(256);
    hipLaunchKernelGGL(zs_build_kernel, gb, tb, 0, st, c->dp.P0, n, n16, rho * (double)m, Mtm.p);
    hipLaunchKernelGGL(zs_pack_sym_kernel, gb, tb, 0, st, (const double *)Mtm.p, Mpk.p, n16);
    hipLaunchKernelGGL(zs_rowsum_kernel, dim3((unsigned)((n16 + 255) / 256)), tb, 0, st, (const double *)Mtm.p, n16, rs.p);
    HIPCHK(c, hipGetLastError());
    std::vector<double> hrs((size_t)n16);
    HIPCHK(c, hipMemcpyAsync(hrs.data(), rs.p, (size_t)n16 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, spin_sync(st));
    double nrm = 0.0;
    for (double v : hrs) nrm = std::max(nrm, v);
    if (!(nrm > 0.0) || !std::isfinite(nrm)) return fail(c, QCQPMI_EINVAL, "admm_zsolver_device: 2 (P0 + rho m I) is zero or not finite");
    hipLaunchKernelGGL(zs_scaled_identity_kernel, gb, tb, 0, st, Xtm.p, n16, 1.0 / nrm);
    double resid = INFINITY, prev = INFINITY;
    int64_t it = 0;
    for (; it < max_iter; it++) {
        hipLaunchKernelGGL(zs_pack_sym_kernel, gb, tb, 0, st, (const double *)Xtm.p, Xpk.p, n16);
        if ((rc = gemm_pk(c, Mpk.p, Xtm.p, Ttm.p, nullptr, KBn, KBn, nt, 1))) return rc;          // T = M X
        if ((rc = gemm_pk(c, Xpk.p, Ttm.p, Utm.p, nullptr, KBn, KBn, nt, 1))) return rc;          // U = X T
        HIPCHK(c, hipMemsetAsync(rb.p, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(zs_update_kernel, gb, tb, 0, st, Xtm.p, (const double *)Utm.p, (const double *)Ttm.p, n16, rb.p);
        HIPCHK(c, hipGetLastError());
        unsigned long long bits = 0;
        HIPCHK(c, hipMemcpyAsync(&bits, rb.p, sizeof bits, hipMemcpyDeviceToHost, st));
        HIPCHK(c, spin_sync(st));
        double r;
        memcpy(&r, &bits, sizeof r);
        prev = resid; resid = r;          // residual of the X this iteration STARTED from; the update squares it
        if (!std::isfinite(resid)) return fail(c, QCQPMI_EREFERENCE, "admm_zsolver_device: iteration diverged (is P0 + rho m I positive definite?)");
        if (resid < 1e-7 && (resid * resid < 1e-15 || resid >= 0.5 * prev)) { it++; break; }   // the update just applied took it to rounding level
        if (it > 8 && resid > 1.0 - 1e-12 && prev > 1.0 - 1e-12 && resid >= prev)
            return fail(c, QCQPMI_EREFERENCE, "admm_zsolver_device: no contraction (is P0 + rho m I positive definite?)");
    }
    if (!(resid < 1e-7)) return fail(c, QCQPMI_EREFERENCE, "admm_zsolver_device: not converged after %lld iterations (residual %.3e)", (long long)it, resid);
    // one refinement step from the converged iterate: X <- X + X (I - M X) with the residual in double-double.  Newton-Schulz in fp64
    // stops at its own rounding (|I - M X| ~ 1e-15 with entries a few ulps off the exact inverse); the step leaves every entry within
    // about an ulp of the exact inverse -- the inverse any other accurate solver (LAPACK, the reference's SuperLU) approximates too
    hipLaunchKernelGGL(zs_pack_sym_kernel, gb, tb, 0, st, (const double *)Xtm.p, Xpk.p, n16);
    hipLaunchKernelGGL(zs_resid_dd_kernel, gb, tb, 0, st, (const double *)Mtm.p, (const double *)Xtm.p, n16, Ttm.p);
    HIPCHK(c, hipGetLastError());
    if ((rc = gemm_pk(c, Xpk.p, Ttm.p, Utm.p, nullptr, KBn, KBn, nt, 1))) return rc;             // U = X R
    hipLaunchKernelGGL(zs_add_kernel, gb, tb, 0, st, Xtm.p, (const double *)Utm.p, tot);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, c->ad_Minvpk.reserve(c->stream, (size_t)tot, false));      // (n16 x n16 whatever rho: reused)
    hipLaunchKernelGGL(zs_pack_sym_kernel, gb, tb, 0, st, (const double *)Xtm.p, c->ad_Minvpk, n16);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, spin_sync(st));
    c->ad_Minv_rho = rho;
    c->ad_Minv_device = true;
    if (resid_out) *resid_out = resid * resid;      // estimate for the final iterate
    if (iters_out) *iters_out = it;
    return 0;
}

// y = P0 v (dense row-major, one wave per row)
__global__ __launch_bounds__(256) void p0_gemv_kernel(const double *__restrict__ P0, const double *__restrict__ v, int64_t n, int64_t n16,
                                                      double *__restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const double *pr = P0 + row * n16;
    double s = 0.0;
    for (int64_t j = lane; j < n; j += 64) s += pr[j] * v[j];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) y[row] = s;
}

// smallest eigenvalue of the symmetric tridiagonal (alpha, beta) by bisection on the Sturm count
static double tridiag_min_eig(const std::vector<double> &al, const std::vector<double> &be, int k) {
    double lo = INFINITY, hi = -INFINITY;
    for (int i = 0; i < k; i++) {
        const double r = (i > 0 ? fabs(be[i - 1]) : 0.0) + (i + 1 < k ? fabs(be[i]) : 0.0);
        lo = std::min(lo, al[i] - r); hi = std::max(hi, al[i] + r);
    }
    auto count_below = [&](double x) {      // eigenvalues < x
        int cnt = 0; double d = 1.0;
        for (int i = 0; i < k; i++) {
            d = al[i] - x - (i > 0 ? be[i - 1] * be[i - 1] / d : 0.0);
            if (d == 0.0) d = -1e-300;
            if (d < 0.0) cnt++;
        }
        return cnt;
    };
    for (int it = 0; it < 200 && hi - lo > 1e-15 * std::max(1.0, std::max(fabs(lo), fabs(hi))); it++) {
        const double mid = 0.5 * (lo + hi);
        if (count_below(mid) >= 1) hi = mid; else lo = mid;
    }
    return 0.5 * (lo + hi);
}

// lambda_min(P0) for the rho check / auto-rho (qcqp.py:262, 272): Lanczos with full reorthogonalisation, products P0 v on
// the device; runs to n steps for small n (exact up to rounding), stops earlier once the Ritz value has settled to `tol`.
int qcqpmi_p0_lambda_min(qcqpmi_ctx *c, int64_t max_steps, double tol, double *lmin_out, int64_t *steps_out) {
    if (!c || !lmin_out) return QCQPMI_EINVAL;
    if (!c->finalized) return fail(c, QCQPMI_ESTATE, "p0_lambda_min: context not finalized");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->n, n16 = c->n16;
    if (c->p0_diag) {
        double v = INFINITY;
        for (int64_t i = 0; i < n; i++) v = std::min(v, c->p0_diag_host[(size_t)i]);
        *lmin_out = v;
        if (steps_out) *steps_out = 0;
        return 0;
    }
    if (max_steps <= 0 || max_steps > n) max_steps = n;
    if (!(tol > 0.0)) tol = 1e-12;
    hipStream_t st = c->stream;
    DevBuf<double> dv, dy;
    HIPCHK(c, dv.reserve(st, (size_t)n16, false));
    HIPCHK(c, dy.reserve(st, (size_t)n16, false));
    std::vector<std::vector<double>> V;
    std::vector<double> al, be, w((size_t)n), v((size_t)n);
    uint64_t sd = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { sd ^= sd << 13; sd ^= sd >> 7; sd ^= sd << 17; return (double)(sd >> 11) / 9007199254740992.0 - 0.5; };
    auto fresh = [&](std::vector<double> &x) {      // random unit vector orthogonal to the basis so far
        for (auto &e : x) e = rnd();
        for (int pass = 0; pass < 2; pass++)
            for (auto &u : V) { double d = 0; for (int64_t i = 0; i < n; i++) d += u[i] * x[i]; for (int64_t i = 0; i < n; i++) x[i] -= d * u[i]; }
        double nr = 0; for (double e : x) nr += e * e; nr = sqrt(nr);
        if (!(nr > 1e-8)) return false;
        for (auto &e : x) e /= nr;
        return true;
    };
    if (!fresh(v)) return fail(c, QCQPMI_EINVAL, "p0_lambda_min: empty problem");
    double theta = INFINITY, scale = 0.0;
    int settled = 0;
    int64_t k = 0;
    for (; k < max_steps; k++) {
        V.push_back(v);
        HIPCHK(c, hipMemcpyAsync(dv.p, v.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(p0_gemv_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, c->dp.P0, (const double *)dv.p, n, n16, dy.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(w.data(), dy.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(c, spin_sync(st));
        double a = 0; for (int64_t i = 0; i < n; i++) a += v[i] * w[i];
        al.push_back(a);
        scale = std::max(scale, fabs(a));
        for (int pass = 0; pass < 2; pass++)       // full reorthogonalisation (twice is enough)
            for (auto &u : V) { double d = 0; for (int64_t i = 0; i < n; i++) d += u[i] * w[i]; for (int64_t i = 0; i < n; i++) w[i] -= d * u[i]; }
        double b = 0; for (double e : w) b += e * e; b = sqrt(b);
        scale = std::max(scale, b);
        const double th = tridiag_min_eig(al, be, (int)al.size());
        if (fabs(th - theta) <= tol * std::max(1.0, scale)) settled++; else settled = 0;
        theta = th;
        if (settled >= 3 && (int64_t)al.size() >= std::min<int64_t>(n, 24)) { k++; break; }
        if ((int64_t)al.size() == n) { k++; break; }
        if (b <= 1e-13 * std::max(1.0, scale)) {      // invariant subspace: continue in its complement
            be.push_back(0.0);
            if (!fresh(v)) { k++; break; }
        } else {
            be.push_back(b);
            for (int64_t i = 0; i < n; i++) v[i] = w[i] / b;
        }
    }
    *lmin_out = theta;
    if (steps_out) *steps_out = k;
    return 0;
}

// The whole run inside ONE persistent kernel (admm_fused.hip) -- reduced bases, diagonal P0.  Returns 1 when the geometry
// does not fit (the caller then takes the multi-launch path), 0 on success, < 0 on errors.
static int admm_run_fused(qcqpmi_ctx *c, int phase1, int64_t num_iters, double tol, double viol_lim, double rho,
                          int64_t *iters1, int64_t *iters2, double *f0_out, double *mv_out) {
    const int64_t n = c->n, n16 = c->n16, m = c->m, R = c->R, Rpad = c->Rpad;
    if (num_iters > 2000000000LL || n16 > (1 << 24) || c->ad_Mh16 > (1 << 24)) return 1;
    AdmmFusedArgs a;
    a.n = (int)n; a.n16 = (int)n16; a.m = (int)m; a.rp = (int)c->ad_rows; a.Mh16 = (int)c->ad_Mh16;
    a.R = (int)R; a.ntiles = (int)(Rpad / 16);
    a.WTpk = c->ad_WTpk; a.Wpk = c->ad_Wpk; a.lam = c->ad_lam; a.qhat = c->ad_qhat; a.rk = c->ad_rk; a.slo = c->ad_slo; a.ehi = c->ad_ehi;
    a.relop = c->ad_relop; a.q0 = c->dp.q0; a.r0 = c->dp.r0; a.rho = rho; a.qzero = c->ad_qzero ? 1 : 0;
    a.phase1 = phase1 ? 1 : 0; a.num_iters = (int)num_iters; a.tol = tol; a.viol_lim = viol_lim; a.sec_tol = 1e-6;
    // workgroups per tile: fill the chip, rows of z per member must fit LDS.  Four-wave workgroups (qcqpmi_admm_fused(ctx, 2)):
    // two workgroups of DIFFERENT tiles share a CU (block b and b + 256 land on one CU: measured), tiles x C fills 2 x CUs.
    int cus = 0;
    HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const int KBn = (int)(n16 / 16);
    int Cmax = 1;
    while (Cmax * 2 <= AF_MAXC && Cmax * 2 <= KBn && Cmax * 2 <= m) Cmax *= 2;
    a.nt = c->ad_fused_nt;
    const int per_cu_want = a.nt == 256 ? 2 : 1;
    int Cwant = 1;
    while (Cwant * 2 <= Cmax && (int64_t)a.ntiles * Cwant * 2 <= (int64_t)cus * per_cu_want) Cwant *= 2;
    a.C = Cwant;
    while (a.C <= Cmax && admm_fused_lds_bytes(a) == 0) a.C *= 2;
    if (a.C > Cmax) return 1;
    int Gmax = admm_fused_max_clusters(a, c->device);
    if (Gmax < 1 && a.nt == 256) { a.nt = 512; Gmax = admm_fused_max_clusters(a, c->device); }
    if (Gmax < 1) return 1;
    a.G = std::min(Gmax, (a.ntiles + 7) / 8 * 8);
    // ---- one work buffer: BEST | xb1 | xb2 | outputs | dinv, pdiag | flags, abort
    const size_t nR = (size_t)n16 * Rpad;
    const size_t n_xb1 = (size_t)a.ntiles * a.C * (a.Mh16 + 2) * 16, n_xb2 = (size_t)a.ntiles * (a.Mh16 + a.C) * 16;
    const size_t n_flags = (size_t)a.ntiles * 2 * a.C + 2;
    const size_t bytes = (nR + n_xb1 + n_xb2 + 4 * (size_t)Rpad + 2 * (size_t)n16) * sizeof(double) + (n_flags + 2) * sizeof(unsigned) + 16 * sizeof(long long);
    hipStream_t st = c->stream;
    HIPCHK(c, c->af_work.reserve(st, bytes, false));
    double *wp = reinterpret_cast<double *>(c->af_work.p);
    a.BEST = wp; wp += nR;
    a.xb1 = wp; wp += n_xb1;
    a.xb2 = wp; wp += n_xb2;
    a.f0_out = wp; wp += Rpad;
    a.mv_out = wp; wp += Rpad;
    a.iters1 = reinterpret_cast<int64_t *>(wp); wp += Rpad;
    a.iters2 = reinterpret_cast<int64_t *>(wp); wp += Rpad;
    double *dinv = wp; wp += n16;
    double *pdiag = wp; wp += n16;
    a.dinv = dinv; a.pdiag = pdiag;
    a.flags = reinterpret_cast<unsigned *>(wp);
    a.abort_flag = reinterpret_cast<int *>(a.flags + (size_t)a.ntiles * 2 * a.C);
    long long *dprof = reinterpret_cast<long long *>(a.flags + ((n_flags + 1) / 2) * 2);
    a.prof = c->profile ? dprof : nullptr;
    if (c->profile) HIPCHK(c, hipMemsetAsync(dprof, 0, 16 * sizeof(long long), st));
    // the operand rows of the padding (and of restarts that never run) must be finite: zero everything the kernel reads
    HIPCHK(c, hipMemsetAsync(a.xb1, 0, (n_xb1 + n_xb2 + 4 * (size_t)Rpad) * sizeof(double), st));
    HIPCHK(c, hipMemsetAsync(a.flags, 0, n_flags * sizeof(unsigned), st));
    {
        std::vector<double> dv((size_t)2 * n16, 0.0);
        for (int64_t j = 0; j < n; j++) {
            dv[(size_t)n16 + j] = c->p0_diag_host[(size_t)j];
            dv[(size_t)j] = 1.0 / (2.0 * (c->p0_diag_host[(size_t)j] + rho * (double)m));      // qcqp.py:224-227 for a diagonal P0
        }
        HIPCHK(c, hipMemcpyAsync(dinv, dv.data(), dv.size() * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(c, spin_sync(st));      // dv goes out of scope
    }
    a.X = c->X;
    tic(c, 4);
    hipError_t le = (hipError_t)admm_fused_launch(a, st);
    toc(c, 4);
    if (le != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, QCQPMI_EHIP, "admm_fused_launch (C = %d, G = %d): %s", a.C, a.G, hipGetErrorString(le));
    }
    c->evaluated = false;
    int ab = 0;
    HIPCHK(c, hipMemcpyAsync(&ab, a.abort_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    if (iters1) HIPCHK(c, hipMemcpyAsync(iters1, a.iters1, (size_t)R * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (iters2) HIPCHK(c, hipMemcpyAsync(iters2, a.iters2, (size_t)R * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (f0_out) HIPCHK(c, hipMemcpyAsync(f0_out, a.f0_out, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, st));
    if (mv_out) HIPCHK(c, hipMemcpyAsync(mv_out, a.mv_out, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, st));
    if (c->profile) HIPCHK(c, hipMemcpyAsync(c->af_prof, dprof, 16 * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, spin_sync(st));
    if (ab) return fail(c, QCQPMI_EHIP, "admm fused kernel: a cluster exchange timed out (C = %d, G = %d)", a.C, a.G);
    c->last_admm_kernel = "admm_fused_kernel";
    c->last_admm_C = a.C;
    return 0;
}

int qcqpmi_admm_fused(qcqpmi_ctx *c, int enable) {
    if (!c) return QCQPMI_EINVAL;
    c->ad_fused = enable != 0;
    c->ad_fused_nt = enable == 2 ? 256 : 512;
    return 0;
}

int qcqpmi_admm_unit_bases(qcqpmi_ctx *c, int enable) {
    if (!c) return QCQPMI_EINVAL;
    c->ad_unit_off = enable == 0;
    return 0;
}

int qcqpmi_debug_admm_profile(qcqpmi_ctx *c, int64_t *out16) {
    if (!c || !out16) return QCQPMI_EINVAL;
    for (int k = 0; k < 16; k++) out16[k] = (int64_t)c->af_prof[k];
    return 0;
}

const char *qcqpmi_last_admm_kernel(qcqpmi_ctx *c, int *workgroups_per_tile) {
    if (workgroups_per_tile) *workgroups_per_tile = c ? c->last_admm_C : 0;
    return c ? c->last_admm_kernel : "";
}

int qcqpmi_admm_run(qcqpmi_ctx *c, int phase1, int64_t num_iters, double tol, double viol_lim, double rho,
                    const double *Minv, int64_t *iters1, int64_t *iters2, double *f0_out, double *mv_out) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!c->ad_WTpk) return fail(c, QCQPMI_ESTATE, "admm_run: qcqpmi_admm_set_eig / set_basis / setup has not been called");
    if (c->ad_fused && c->ad_lowrank && c->ad_rows >= 2 && c->ad_rows <= AF_MAXRP && c->p0_diag && !Minv && num_iters >= 0) {
        HIPCHK(c, hipSetDevice(c->device));
        rc = admm_run_fused(c, phase1, num_iters, tol, viol_lim, rho, iters1, iters2, f0_out, mv_out);
        if (rc <= 0) return rc;      // done (or failed); 1: geometry does not fit -> the multi-launch path below
    }
    c->last_admm_kernel = (c->ad_unit && !c->ad_unit_off) ? "admm_multi_launch<unit bases>" : "admm_multi_launch";
    c->last_admm_C = 0;
    const bool dev_minv = !Minv && !c->p0_diag && c->ad_Minv_device && c->ad_Minvpk && c->ad_Minv_rho == rho;
    if (!Minv && !c->p0_diag && !dev_minv)
        return fail(c, QCQPMI_EINVAL, "admm_run: Minv missing (it may only be omitted when P0 is diagonal or after qcqpmi_admm_zsolver_device with the same rho)");
    if (c->ad_rows > 16384) return fail(c, QCQPMI_EUNSUPPORTED, "admm: more than 16384 basis rows per constraint (full eigenbasis at n > 16384); use reduced bases (qcqpmi_admm_set_basis)");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->n, n16 = c->n16, m = c->m, R = c->R, Rpad = c->Rpad, Mh16 = c->ad_Mh16;
    const int ntiles = (int)(Rpad / 16), KBn = (int)(n16 / 16), MBh = (int)(Mh16 / 16);
    hipStream_t st = c->stream;
    // ---- work arrays (tile-major like the population)
    DevBuf<double> X0, Z, Zlast, Znew, Sp, Y, BEST, ZQ, UH, dist2, f0z, bf0, bmv, fa, dinv, pdiag;
    DevBuf<unsigned long long> mvb;
    DevBuf<uint8_t> act, pick;
    DevBuf<int64_t> it1, it2;
    DevBuf<int> nact;
    const size_t nR = (size_t)n16 * Rpad;
    const bool unit = c->ad_unit && !c->ad_unit_off;      // unit bases: gather / scatter instead of the two consensus GEMMs
    const int zs2 = unit ? 1 : gemm_zsplit(KBn, ntiles, MBh);       // planes of S = W D
    HIPCHK(c, X0.reserve(c->stream, nR));
    HIPCHK(c, Z.reserve(c->stream, nR));
    HIPCHK(c, Zlast.reserve(c->stream, nR));
    HIPCHK(c, Znew.reserve(c->stream, nR));
    HIPCHK(c, Sp.reserve(c->stream, nR * (size_t)zs2));
    HIPCHK(c, Y.reserve(c->stream, nR));
    HIPCHK(c, BEST.reserve(c->stream, nR));
    // ZQ = W^T Z has few rows in a reduced basis (m rp): split the contraction over n into planes the small secular kernel sums
    const int zs1 = unit ? 1 : (c->ad_lowrank && c->ad_rows <= 8) ? gemm_zsplit(MBh, ntiles, KBn) : 1;
    HIPCHK(c, ZQ.reserve(c->stream, (size_t)Mh16 * Rpad * (size_t)zs1));
    HIPCHK(c, UH.reserve(c->stream, (size_t)Mh16 * Rpad));
    HIPCHK(c, dist2.reserve(c->stream, Rpad));
    HIPCHK(c, f0z.reserve(c->stream, Rpad));
    HIPCHK(c, bf0.reserve(c->stream, Rpad));
    HIPCHK(c, bmv.reserve(c->stream, Rpad));
    HIPCHK(c, fa.reserve(c->stream, Rpad));
    HIPCHK(c, mvb.reserve(c->stream, Rpad));
    HIPCHK(c, act.reserve(c->stream, Rpad));
    HIPCHK(c, pick.reserve(c->stream, Rpad));
    HIPCHK(c, it1.reserve(c->stream, Rpad));
    HIPCHK(c, it2.reserve(c->stream, Rpad));
    HIPCHK(c, nact.reserve(c->stream, 8));         // one counter of active restarts per iteration, eight iterations between two host reads
    // ---- the z-solve (qcqp.py:224-227, 231-232): (2 (P0 + rho m I))^-1 given by the host, packed for the GEMM -- or, for a
    // diagonal P0, formed right here
    const bool diag = !Minv && !dev_minv;
    const bool f0_identity = !diag && !(c->dbg & 4);       // phase 2: f0(z) from the solve's own right-hand side (admm_take_z_kernel); debug bit 4: the product with P0
    if (dev_minv) {
        // (2 (P0 + rho m I))^-1 was formed on the device: nothing to upload
    } else if (diag) {
        std::vector<double> dv((size_t)n16, 0.0), pd((size_t)n16, 0.0);
        for (int64_t j = 0; j < n; j++) { pd[(size_t)j] = c->p0_diag_host[(size_t)j]; dv[(size_t)j] = 1.0 / (2.0 * (pd[(size_t)j] + rho * (double)m)); }
        HIPCHK(c, dinv.reserve(c->stream, (size_t)n16, false));
        HIPCHK(c, pdiag.reserve(c->stream, (size_t)n16, false));
        HIPCHK(c, hipMemcpyAsync(dinv.p, dv.data(), (size_t)n16 * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(pdiag.p, pd.data(), (size_t)n16 * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(c, spin_sync(st));
    } else {
        DevBuf<double> tmp;
        HIPCHK(c, tmp.reserve(c->stream, (size_t)n * n, false));
        HIPCHK(c, hipMemcpyAsync(tmp.p, Minv, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, st));
        c->ad_Minv_device = false;
        HIPCHK(c, c->ad_Minvpk.reserve(c->stream, (size_t)n16 * n16, false));
        const int64_t tot = n16 * n16;
        hipLaunchKernelGGL(gemm_pk_pack_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const double *)tmp.p, c->ad_Minvpk, n, n, n, (int64_t)1, KBn, KBn);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, spin_sync(st));
    }
    // population -> X0 (same layout: a copy)
    HIPCHK(c, hipMemcpyAsync(X0.p, c->X, nR * sizeof(double), hipMemcpyDeviceToDevice, st));
    const unsigned gNR = (unsigned)((nR + 255) / 256);
    AdmmArgs sa;
    admm_fill_args(c, sa, R);
    sa.ZQ = ZQ.p; sa.UH = UH.p; sa.act = act.p; sa.mvbits = mvb.p;
    sa.zq_planes = zs1; sa.zq_plane = (int64_t)Mh16 * Rpad;
    auto gemm1 = [&](const double *Zin) -> int {   // ZQ = W^T Zin
        if (unit) {
            const int64_t tot = (int64_t)ntiles * Mh16 * 16;
            hipLaunchKernelGGL(admm_unit_gather_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, Zin, ZQ.p, (const int *)c->ad_uidx,
                               (const double *)c->ad_usgn, n16, Mh16, tot);
            HIPCHK(c, hipGetLastError());
            return 0;
        }
        return gemm_pk(c, c->ad_WTpk, Zin, ZQ.p, nullptr, MBh, KBn, ntiles, zs1);
    };
    // the max violations start from zero: a fill before an evaluation and before the first iteration of a phase; admm_book_kernel
    // leaves them zeroed for the iteration that follows it
    auto secular = [&](int first_iter, int viol_only) -> int {
        if (first_iter) HIPCHK(c, hipMemsetAsync(mvb.p, 0, (size_t)Rpad * sizeof(unsigned long long), st));
        sa.first_iter = first_iter; sa.viol_only = viol_only;
        return admm_launch_secular(c, sa);
    };
    auto gemm2 = [&]() -> int {                    // S planes = W D  (K = m rows: split over grid.z)
        if (unit) {
            const int64_t tot = (int64_t)ntiles * n16 * 16;
            hipLaunchKernelGGL(admm_unit_scatter_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const double *)ZQ.p, Sp.p,
                               (const int *)c->ad_uptr, (const int *)c->ad_ulist, (const double *)c->ad_usgn, n16, Mh16, tot);
            HIPCHK(c, hipGetLastError());
            return 0;
        }
        return gemm_pk(c, c->ad_Wpk, ZQ.p, Sp.p, nullptr, KBn, MBh, ntiles, zs2);
    };
    // unit bases with one row per constraint: gather + projection + scatter of an iteration in one launch (admm_unit_step_kernel);
    // debug bit 2: the three launches it replaces (same bits: the cross-check of the tests)
    const bool unit1 = unit && c->ad_rows == 1 && zs1 == 1 && zs2 == 1 && !(c->dbg & 2);
    // zmode 1: phase 1, the z-update in front (no admm_zupdate_kernel launch); 2: phase 2 with a dense solve, the next right-hand side behind
    auto unit_step = [&](double *Zio, int first_iter, int zmode) -> int {
        if (first_iter) HIPCHK(c, hipMemsetAsync(mvb.p, 0, (size_t)Rpad * sizeof(unsigned long long), st));
        sa.first_iter = first_iter; sa.viol_only = 0;
        const int64_t tot = (int64_t)ntiles * n16 * 16;
        tic(c, 4);
        hipLaunchKernelGGL(admm_unit_step_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, sa, Zio, Sp.p, (const int *)c->ad_uptr,
                           (const int *)c->ad_ulist, (const double *)c->ad_usgn, n16, tot, zmode, c->ad_lowrank ? 1 : 0, (double)m, rho,
                           (const double *)c->dp.q0, Y.p, n);
        toc(c, 4);
        HIPCHK(c, hipGetLastError());
        return 0;
    };
    AdmmZArgs za;
    za.n = n; za.n16 = n16; za.R = R; za.zs = zs2; za.plane = (int64_t)nR; za.add_mz = c->ad_lowrank; za.m = (double)m; za.rho = rho;
    za.Sp = Sp.p; za.Z = Z.p; za.Y = Y.p; za.q0 = c->dp.q0; za.dinv = diag ? dinv.p : nullptr; za.Zlast = Zlast.p;
    za.dist2 = dist2.p; za.act = act.p;
    za.pdiag = nullptr; za.r0 = c->dp.r0; za.f0z = f0z.p;
    auto f0_of = [&](const double *Zin, double *out) -> int {   // f0 = z^T P0 z + q0^T z + r0
        if (!diag) { int r_ = gemm_pk(c, c->dp.Apack, Zin, Y.p, nullptr, KBn, KBn, ntiles, 1); if (r_) return r_; }
        hipLaunchKernelGGL(admm_f0_kernel, dim3((unsigned)ntiles), dim3(ADMM_TPB), 0, st, Zin, (const double *)Y.p, diag ? (const double *)pdiag.p : (const double *)nullptr,
                           c->dp.q0, c->dp.r0, out, n, n16, R);
        HIPCHK(c, hipGetLastError());
        return 0;
    };
    // (f0, max violation) of a set of points, in the arithmetic the iteration itself uses
    auto evaluate = [&](const double *Zin, double *f_dev, std::vector<double> &fh, std::vector<double> &vh) -> int {
        int r_;
        HIPCHK(c, hipMemsetAsync(act.p, 1, (size_t)Rpad, st));
        if ((r_ = gemm1(Zin))) return r_;
        if ((r_ = secular(1, 1))) return r_;
        if ((r_ = f0_of(Zin, f_dev))) return r_;
        std::vector<unsigned long long> bits((size_t)R);
        fh.resize((size_t)R); vh.resize((size_t)R);
        HIPCHK(c, hipMemcpyAsync(fh.data(), f_dev, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(bits.data(), mvb.p, (size_t)R * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPCHK(c, spin_sync(st));
        for (int64_t r = 0; r < R; r++) memcpy(&vh[(size_t)r], &bits[(size_t)r], 8);
        return 0;
    };
    auto better_first = [&](double f1, double v1, double f2, double v2) {   // does QCQPForm.better return its FIRST argument?
        long long b1 = (long long)(v1 / 1e-4), b2 = (long long)(v2 / 1e-4);
        if (b1 < b2) return true;
        if (b2 < b1) return false;
        return f1 < f2;
    };
    auto count_active = [&](int *out, int64_t t) -> int {
        HIPCHK(c, hipMemcpyAsync(out, nact.p + (t & 7), sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(c, spin_sync(st));
        return 0;
    };
    AdmmBook bk;
    bk.n = n; bk.n16 = n16; bk.R = R; bk.tol = tol; bk.viol_lim = viol_lim; bk.Z = Z.p; bk.Zlast = Zlast.p; bk.BEST = BEST.p;
    bk.dist2 = dist2.p; bk.f0z = f0z.p; bk.mvbits = mvb.p; bk.best_f0 = bf0.p; bk.best_mv = bmv.p; bk.act = act.p;
    bk.nactive = nact.p; bk.first = 0; bk.X0 = X0.p;
    // first z-update of a phase: xs = x0, us = 0  =>  S = m x0.  In a reduced basis S is assembled as m z + W D: the
    // planes hold zero then.
    auto seed_S = [&](const double *x) -> int {
        if (c->ad_lowrank) HIPCHK(c, hipMemsetAsync(Sp.p, 0, nR * (size_t)zs2 * sizeof(double), st));
        else {
            if (zs2 > 1) HIPCHK(c, hipMemsetAsync(Sp.p + nR, 0, nR * (size_t)(zs2 - 1) * sizeof(double), st));
            hipLaunchKernelGGL(admm_scale_kernel, dim3(gNR), dim3(256), 0, st, Sp.p, x, (int64_t)nR, (double)m);
            HIPCHK(c, hipGetLastError());
        }
        return 0;
    };

    std::vector<double> f_x0, v_x0, f_a, v_a;
    if ((rc = evaluate(X0.p, fa.p, f_x0, v_x0))) return rc;
    std::vector<uint8_t> pk((size_t)Rpad, 0);
    // ================================================================ phase 1 (qcqp.py:195-212)
    std::vector<double> f_x1 = f_x0, v_x1 = v_x0;
    if (phase1) {
        HIPCHK(c, hipMemcpyAsync(Z.p, X0.p, nR * sizeof(double), hipMemcpyDeviceToDevice, st));
        if ((rc = seed_S(X0.p))) return rc;
        HIPCHK(c, hipMemsetAsync(act.p, 1, (size_t)Rpad, st));
        bk.phase = 1; bk.iters = it1.p; bk.have_last = 0;
        za.phase = 1;
        for (int64_t t = 0; t < num_iters; t++) {
            if (unit1) { if ((rc = unit_step(Z.p, t == 0, 1))) return rc; }        // z = (sum xs - sum us) / m inside
            else {
                hipLaunchKernelGGL(admm_zupdate_kernel, dim3((unsigned)ntiles), dim3(ADMM_TPB), 0, st, za);   // z = (sum xs - sum us) / m
                if ((rc = gemm1(Z.p))) return rc;
                if ((rc = secular(t == 0, 0))) return rc;
                if ((rc = gemm2())) return rc;
            }
            if ((t & 7) == 0) HIPCHK(c, hipMemsetAsync(nact.p, 0, 8 * sizeof(int), st));
            bk.nactive = nact.p + (t & 7);
            bk.first = t == 0 ? 1 : 0;
            hipLaunchKernelGGL(admm_book_kernel, dim3((unsigned)ntiles), dim3(ADMM_TPB), 0, st, bk);
            HIPCHK(c, hipGetLastError());
            if ((t & 7) == 7 || t + 1 == num_iters) {
                int na = 0;
                if ((rc = count_active(&na, t))) return rc;
                if (na == 0) break;
            }
        }
        bk.first = 0;
        // x1 = better(x0, z1) (qcqp.py:281)
        if ((rc = evaluate(Z.p, fa.p, f_a, v_a))) return rc;
        for (int64_t r = 0; r < R; r++) {
            bool first = better_first(f_x0[(size_t)r], v_x0[(size_t)r], f_a[(size_t)r], v_a[(size_t)r]);
            pk[(size_t)r] = first ? 1 : 0;
            if (!first) { f_x1[(size_t)r] = f_a[(size_t)r]; v_x1[(size_t)r] = v_a[(size_t)r]; }
        }
        HIPCHK(c, hipMemcpyAsync(pick.p, pk.data(), (size_t)Rpad, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(admm_select_cols_kernel, dim3(gNR), dim3(256), 0, st, Znew.p, (const double *)X0.p, (const double *)Z.p, (const uint8_t *)pick.p, n16, R, (int64_t)nR);
        HIPCHK(c, hipMemcpyAsync(X0.p, Znew.p, nR * sizeof(double), hipMemcpyDeviceToDevice, st));   // X0 now holds x1
        HIPCHK(c, spin_sync(st));
    }
    const double *x1 = X0.p;     // the point phase 2 starts from
    // ================================================================ phase 2 (qcqp.py:215-251)
    HIPCHK(c, hipMemcpyAsync(Z.p, x1, nR * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(Zlast.p, x1, nR * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(BEST.p, x1, nR * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(bf0.p, f_x1.data(), (size_t)R * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(bmv.p, v_x1.data(), (size_t)R * sizeof(double), hipMemcpyHostToDevice, st));
    if ((rc = seed_S(x1))) return rc;
    HIPCHK(c, hipMemsetAsync(act.p, 1, (size_t)Rpad, st));
    bk.phase = 2; bk.iters = it2.p;
    za.phase = 2;
    za.pdiag = diag ? pdiag.p : nullptr;      // diagonal P0: the z-update pass also leaves f0(z)
    for (int64_t t = 0; t < num_iters; t++) {
        const bool rhs_behind = unit1 && !diag && f0_identity;      // the unit step of iteration t - 1 left the right-hand side of this solve in Y (f0 through the product with P0 uses Y as its scratch)
        if (!rhs_behind || t == 0)
            hipLaunchKernelGGL(admm_zupdate_kernel, dim3((unsigned)ntiles), dim3(ADMM_TPB), 0, st, za);   // rhs, and z itself when the solve is diagonal
        if (!diag) {
            if ((rc = gemm_pk(c, c->ad_Minvpk, Y.p, Znew.p, nullptr, KBn, KBn, ntiles, 1))) return rc;
            hipLaunchKernelGGL(admm_take_z_kernel, dim3((unsigned)ntiles), dim3(ADMM_TPB), 0, st, Z.p, (const double *)Znew.p, (const double *)Zlast.p,
                               (const uint8_t *)act.p, dist2.p, n, n16, R, f0_identity ? (const double *)Y.p : (const double *)nullptr,
                               (const double *)c->dp.q0, c->dp.r0, rho * (double)m, f0z.p);
        }
        if (unit1) { if ((rc = unit_step(Z.p, t == 0, rhs_behind ? 2 : 0))) return rc; }
        else {
            if ((rc = gemm1(Z.p))) return rc;
            if ((rc = secular(t == 0, 0))) return rc;
            if ((rc = gemm2())) return rc;
        }
        if (!diag && !f0_identity && (rc = f0_of(Z.p, f0z.p))) return rc;      // (diagonal P0: f0 came out of the z-update pass; dense: out of the solve)
        bk.have_last = t > 0 ? 1 : 0;
        if ((t & 7) == 0) HIPCHK(c, hipMemsetAsync(nact.p, 0, 8 * sizeof(int), st));
        bk.nactive = nact.p + (t & 7);
        hipLaunchKernelGGL(admm_book_kernel, dim3((unsigned)ntiles), dim3(ADMM_TPB), 0, st, bk);
        HIPCHK(c, hipGetLastError());
        if ((t & 7) == 7 || t + 1 == num_iters) {
            int na = 0;
            if ((rc = count_active(&na, t))) return rc;
            if (na == 0) break;
        }
    }
    // The loop's f0(z) came from the solve's right-hand side when f0_identity: exact only to the accuracy of (2 (P0 + rho m I))^-1
    // as supplied (host) or iterated (Newton-Schulz).  What is REPORTED and compared below is f0 of the best point through P0
    // itself (one product per run) -- the same arithmetic as f_x1 (evaluate -> f0_of).
    if (f0_identity && (rc = f0_of(BEST.p, bf0.p))) return rc;
    // x2 = better(x1, bestx) (qcqp.py:284)
    std::vector<double> f_b((size_t)R), v_b((size_t)R);
    HIPCHK(c, hipMemcpyAsync(f_b.data(), bf0.p, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(v_b.data(), bmv.p, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, spin_sync(st));
    for (int64_t r = 0; r < R; r++) {
        bool first = better_first(f_x1[(size_t)r], v_x1[(size_t)r], f_b[(size_t)r], v_b[(size_t)r]);
        pk[(size_t)r] = first ? 1 : 0;
        if (first) { f_b[(size_t)r] = f_x1[(size_t)r]; v_b[(size_t)r] = v_x1[(size_t)r]; }
    }
    HIPCHK(c, hipMemcpyAsync(pick.p, pk.data(), (size_t)Rpad, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(admm_select_cols_kernel, dim3(gNR), dim3(256), 0, st, c->X, x1, (const double *)BEST.p, (const uint8_t *)pick.p, n16, R, (int64_t)nR);
    HIPCHK(c, hipGetLastError());
    c->evaluated = false;
    if (iters1) HIPCHK(c, hipMemcpyAsync(iters1, it1.p, (size_t)R * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (iters2) HIPCHK(c, hipMemcpyAsync(iters2, it2.p, (size_t)R * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, spin_sync(st));
    if (f0_out) memcpy(f0_out, f_b.data(), (size_t)R * sizeof(double));
    if (mv_out) memcpy(mv_out, v_b.data(), (size_t)R * sizeof(double));
    return 0;
}

}  // extern "C"
