// Internal header of the host side of the C ABI: what two or more of its units (capi.hip, capi_cd.hip, capi_dense.hip, capi_admm.hip,
// capi_small.hip, capi_units.hip, capi_comm.hip, capi_stream.hip) need, and nothing else -- the context, the error slot, the event timers
// and the few host functions one unit calls in another.  Types and host declarations only: no kernel is defined in anything included here,
// so a unit that includes it compiles device code only for the kernel headers it names itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/qcqp_mi.h"
#include "kernels.h"      // DevProblem
#include "cd_queue.h"     // CdLife, CdBatch
#include "dev_buf.h"

typedef struct ncclComm *ncclComm_t;      // as rccl/rccl.h declares it: only capi_comm.hip includes that header

namespace qcqpmi {

struct HostQuad {
    bool set = false;
    std::vector<int> ci, cj;  // COO
    std::vector<double> cv;
    std::vector<double> q;
    double r = 0.0;
    int relop = 0;
    // generated on the device (qcqpmi_set_quad_generated)
    bool gen = false;
    uint64_t gseed = 0;
    double gscale = 0.0, gqscale = 0.0, gdiag = 0.0;
    // packed on the device at qcqpmi_set_quad time (problems whose constraint matrices exceed the row-major budget)
    bool streamed = false;
};

struct Timer {
    hipEvent_t beg = nullptr, end = nullptr;
    bool valid = false;
};

}  // namespace qcqpmi

// Every device or pinned pointer the context OWNS is a DevBuf / PinBuf (dev_buf.h): freed when the context is deleted, grown with
// reserve().  Raw pointers below only view another allocation (dn_Gpack, dn_q, ..., dp.*: all of them in prob_allocs).
struct qcqpmi_ctx {
    int device = 0;
    int64_t n = 0, n16 = 0, m = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::vector<qcqpmi::HostQuad> quads;  // m+1
    bool finalized = false;
    bool sep = false;
    int maxc = 0;
    int K = 0;
    int objclass = 0;  // 1: every P0[i,i] > 0, 2: every P0[i,i] == 0, 0: mixed (negative entries, or zero in places: cd_life_kernel's SGN kind)
    bool symcls = false;  // one constraint class of the form p x_i^2 + r == 0 (feasible sets mirrored about 0)
    qcqpmi::DevProblem dp{};
    std::vector<DevBuf<char>> prob_allocs;   // the problem's arrays (dp.*, dn_*, d_gP): allocated at finalize, never grown
    // population: the group below grows together (pop_reserve, Rcap restarts); Xi and d_F are sized on demand and dropped with it
    int64_t R = 0, Rpad = 0, Rcap = 0;
    DevBuf<double> X, Xi;        // Xi: the standard normals of pop_sdr_sample
    DevBuf<double> d_f0, d_mv, d_F;
    DevBuf<int64_t> d_visits, d_acc, d_sweeps, d_sweeps1;
    DevBuf<int> d_status, d_status1;
    DevBuf<uint8_t> d_flag;
    DevBuf<int64_t> d_best_idx;
    DevBuf<double> d_best_key;
    DevBuf<double> d_stage;  // host-layout staging (n x Rcap)
    bool evaluated = false;
    // SDR factor
    DevBuf<double> d_Fpack, d_Frow, d_mu;
    qcqpmi::Timer timers[5];
    // ADMM: the stacked bases B = [B_1 ... B_m] packed for the two products (gemm_pk.h), eigenvalues, B^T q, brackets
    // unit bases (every basis vector is +-e_i: separable constraints): ZQ = W^T Z is a gather, S = W D a scatter (no GEMM)
    DevBuf<int> ad_uidx, ad_uptr, ad_ulist;                                // [Mh16] coordinate of basis row h (-1: padding); CSR coordinate -> rows
    DevBuf<double> ad_usgn;                                                // [Mh16] its sign
    bool ad_unit = false, ad_unit_off = false;
    DevBuf<double> ad_WTpk, ad_Wpk, ad_lam, ad_qhat, ad_rk, ad_slo, ad_ehi;
    DevBuf<double> ad_Minvpk;
    DevBuf<int> ad_relop;
    int64_t ad_rows = 0, ad_Mh16 = 0;   // hat rows per constraint (n, or rp of a reduced basis); m * rows padded to 16
    int ad_lowrank = 0;
    bool ad_qzero = false;              // every B_k^T q_k is zero
    void *rb_handle = nullptr;          // rocBLAS handle: only the rocSOLVER setup path needs one
    bool p0_diag = false;               // P0 has no off-diagonal entries (z-update and f0 need no product then)
    std::vector<double> p0_diag_host;
    // outputs of a run packed into one device buffer, copied with ONE transfer into pinned host memory
    DevBuf<char> d_out;
    PinBuf<char> h_out;
    PinBuf<char> h_pin;                   // pinned bounce buffer of the relaxation solver's downloads
    int eval_zs = 1;   // planes of the last dense evaluation
    DevBuf<double> d_wS, d_wY, d_ww, d_wz;   // qcqpmi_pop_weighted_product work buffers
    DevBuf<double> d_planes;   // partial planes of x'P0x from the GEMM evaluation
    double *d_gP = nullptr;   // dense constraint matrices [m][n][n] (problems whose constraints couple coordinates): in prob_allocs
    // dense-constraint path (cd_dense.h): all matrices in block-major fragment order + work buffers
    const double *dn_Gpack = nullptr, *dn_q = nullptr, *dn_qT = nullptr, *dn_r = nullptr;
    const int *dn_relop = nullptr;
    DevBuf<double> dn_G, dn_Dg, dn_Ft;    // dn_Ft grows with dn_G
    int dense_chain_mode = 0;             // 0: four waves per restart where it applies, 1: one wave per restart (cross-check)
    DevBuf<long long> dn_prof;            // 32 tick sums of the dense chain kernel (debug profile)
    DevBuf<char> dn_state;                // per-restart state of a dense phase (dense_state lays it out for Rpad restarts)
    hipStream_t stream2 = nullptr;   // second stream of the dense path: products of block b+1 while the chain walks b
    hipEvent_t dn_ev[3] = {nullptr, nullptr, nullptr};
    hipEvent_t dn_evn[2] = {nullptr, nullptr};   // "live count of sweep t copied" (dense path: the host runs one sweep ahead)
    PinBuf<int> dn_hn;                           // pinned: the two live counts in flight
    bool dn_force = false;    // generated functions: the dense path is the only one that holds them
    // streaming upload (coupled constraints beyond `stream_limit` bytes of row-major storage): every function is packed for the
    // matrix cores as it arrives; neither the host nor the device ever holds a second copy
    double stream_limit = 16e9;
    DevBuf<double> dn_gp_pre, dn_tmp;     // the packed matrices until finalize takes them over; the row-major staging of one function
    // comm
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    DevBuf<double> d_comm, d_comm_big;
    DevBuf<long long> d_prof;
    int cd_stage = 0;                   // qcqpmi_cd_run_stage: last stage completed of a split run
    bool sdr_factor_resident = false;   // d_Fpack / d_mu hold the pair of the last pop_sdr_sample
    double ad_Minv_rho = 0.0;           // rho of the z-solver matrix formed by qcqpmi_admm_zsolver_device
    bool ad_Minv_device = false;
    const char *last_cd2_kernel = "";     // name of the phase-2 kernel of the most recent cd run (bench / profiles)
    bool profile = false;
    int dbg = 0;
    // fused persistent ADMM kernel (admm_fused.h): one work buffer kept across runs, grown on demand
    DevBuf<char> af_work;
    bool ad_fused = true;                 // qcqpmi_admm_fused: use the fused kernel where it applies
    int ad_fused_nt = 512;                // threads per workgroup of the fused kernel (256: qcqpmi_admm_fused(ctx, 2))
    const char *last_admm_kernel = "";    // "admm_fused_kernel" / "admm_multi_launch"
    int last_admm_C = 0;                  // workgroups per tile of the last fused run
    long long af_prof[16] = {0};          // stage cycle counters of the last fused run (when qcqpmi_debug_profile enabled them)
    int cd_queue = 2;                     // qcqpmi_cd_queue: 0 off, 1 restart-level scheduling (cd_phase2_qs_kernel) wherever it applies,
                                          // 2 auto: when there are more tiles than CUs
    DevBuf<int> d_qnext;                  // [0] queue head of the slot-queue kernel
    bool q_prepared = false;              // the queue of the resident population has been reset
    DevBuf<qcqpmi::CdLife> d_life;       // qcqpmi_cd_stream_run: parameters of the lifecycle launch
    // second-generation lifecycle kernel (cd_life.h): the workgroups' X tiles, the staged diagonal blocks, the watchdog word
    int Kreal = 0;               // constraint classes among the REAL coordinates (the padded ones of n16 carry no constraint)
    double fbound = 0.0;         // sum |P0| + sum |q0| + |r0|
    DevBuf<double> l2_scratch;
    DevBuf<double> l2_D, l2_S;
    DevBuf<int> l2_abort;
    DevBuf<int> l2_cuslot;       // [4096] arrival counters per compute unit of cd_life_kernel (zeroed before every launch)
    DevBuf<double> l2_preslack;  // [K R] slack of the prebuilt columns (cd_life2_prep_launch)
    DevBuf<double> l2_y0;        // [tile][16 lr_RB][16] Y0 = L^T x0 of the preloaded restarts (cd_life2_y0_launch)
    // factored objective P0 = L L^T (qcqpmi_cd_set_objective_factor): L (n16 x 16 lr_RB, zero-padded) and its fragment packs
    DevBuf<double> lr_L, lr_G, lr_U; int lr_RB = 0;
    int life_version = 0;        // qcqpmi_cd_life_version: 0 = the faster one for the shape, 2 = cd_life_kernel wherever it applies, 1 = cd_phase2_qs_kernel<lifecycle> only
    DevBuf<long long> d_life_prof;
    DevBuf<int64_t> d_bestK_idx; DevBuf<double> d_bestK_key, d_bestK_x;
    bool cd_ref_order = false;   // qcqpmi_cd_reference_order: coupled constraints in the reference's summation order
    bool force_generic = false;  // debug/tests: run the general phase-2 kernel even when the pipelined one applies
    std::vector<int> last_st1, last_st2;   // per-restart status codes of the last coordinate-descent run (qcqpmi_cd_status)
    // capi_small.hip, the CD and ADMM batch calls: ONE device buffer for the objectives, starts, per-restart outputs, points and winners
    // of a call (grown on demand; the resident population and its buffers are never used by that call)
    DevBuf<char> sb_work;
    // qcqpmi_sdr_small_batch: d (n) when every coordinate carries exactly one constraint p x_i^2 + r == 0 with d_i = -r / p > 0 (the
    // unit-diagonal family of the relaxation), else empty; and the call's own device buffer, like sb_work
    std::vector<double> unit_d;
    DevBuf<char> ss_work;
};

namespace qcqpmi {

// capi.hip: the message goes to the context, or without one to the thread's slot that qcqpmi_last_error(NULL) reads
int fail(qcqpmi_ctx *c, int code, const char *fmt, ...);

#define HIPCHK(c, expr)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(c, QCQPMI_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                  \
    } while (0)

int check_ready(qcqpmi_ctx *c, bool need_pop);      // capi.hip

inline void tic(qcqpmi_ctx *c, int which) { (void)hipEventRecord(c->timers[which].beg, c->stream); }
inline void toc(qcqpmi_ctx *c, int which) {
    (void)hipEventRecord(c->timers[which].end, c->stream);
    c->timers[which].valid = true;
}

// `count` elements of the problem's own storage: owned by prob_allocs until the context goes (qcqpmi_finalize, and dense_build of
// capi_dense.hip for the packed matrices and their vectors)
template <typename T>
int prob_alloc(qcqpmi_ctx *c, T **dst, size_t count) {
    DevBuf<char> b;
    HIPCHK(c, b.reserve(c->stream, std::max<size_t>(count, 1) * sizeof(T), false));
    *dst = (T *)b.p;
    c->prob_allocs.push_back(std::move(b));
    return 0;
}

template <typename T>
int prob_upload(qcqpmi_ctx *c, const T **dst, const std::vector<T> &src) {
    T *p = nullptr;
    int rc = prob_alloc(c, &p, src.size());
    if (rc) return rc;
    if (!src.empty())
        HIPCHK(c, hipMemcpyAsync(p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *dst = p;
    return 0;
}

// Launches of the kernels of kernels_impl.h that a unit other than capi.hip needs: enqueued on c->stream, no wait (the
// caller checks hipGetLastError as after any launch).
// capi.hip: one workgroup per population of R restarts selects its best (out_idx[2 p], out_key[2 p]: select_best_kernel)
void launch_select_best(qcqpmi_ctx *c, int64_t pops, const double *f0, const double *maxviol, int64_t R, double tol, int64_t *out_idx,
                        double *out_key);
// capi.hip: R restarts of the tile-major array Xt -> c->d_stage in the host's layout (from_tiles_kernel)
void launch_from_tiles(qcqpmi_ctx *c, const double *Xt, int64_t R);
// capi.hip: the columns idx[2 p] of `pops` populations of R restarts of the resident population -> out [pops][n] (gather_best_x_kernel)
void launch_gather_best_x(qcqpmi_ctx *c, int64_t pops, int64_t R, const int64_t *idx, double *out);
// capi.hip: objective and max violation of the resident population into d_f0 / d_mv, every function value into d_F when want_F
// (eval_kernel, behind the planes GEMM from 8 row blocks x 8 tiles; the dense path's launch_eval_dense where dense_on); timer 0
int launch_eval(qcqpmi_ctx *c, bool want_F);
// capi.hip: the resident population's buffers for R restarts
int pop_reserve(qcqpmi_ctx *c, int64_t R);

// capi_cd.hip, for the streamed run of capi_stream.hip and the dense run of capi_dense.hip: the staging buffers of fetch_cd_outputs;
// the per-restart results of a run -> host (one transfer, one wait) and the status policy on them; the restarts a queue launch works
// on; the shape rule of the round-4 slot-queue kernel; the gate of improve_coord_descent on d_mv / d_status1 -> d_flag (gate_kernel:
// enqueued, no wait)
int cd_outputs_reserve(qcqpmi_ctx *c, int64_t R);
int fetch_cd_outputs(qcqpmi_ctx *c, int64_t *sweeps1, int64_t *sweeps2, int64_t *visits2, int64_t *accepted2, uint8_t *ran_phase2,
                     double *f0, double *maxviol, std::vector<int> &st, std::vector<int> &st1);
int cd_apply_status(qcqpmi_ctx *c, const std::vector<int> &st, const std::vector<int> &st1, double *f0, double *maxviol, int seg_cap);
void cd_queue_fill_batch(qcqpmi_ctx *c, CdBatch &B, uint64_t seed, uint64_t first_index);
bool cd_queue_shape_ok(const qcqpmi_ctx *c);
void launch_gate(qcqpmi_ctx *c, double viol_tol);

// capi_dense.hip, the dense-constraint path (the kernels of cd_dense.h and cd_dense_mw.h).  Does the problem take it; the name of its
// chain kernel; its evaluation (every function on the matrix cores; with_Ft: the tracked values too) and its coordinate descent
bool dense_on(const qcqpmi_ctx *c);
const char *dense_chain_name(const qcqpmi_ctx *c);
int launch_eval_dense(qcqpmi_ctx *c, bool with_Ft);
int cd_run_dense(qcqpmi_ctx *c, int phase1, int64_t num_iters, double viol_tol, double tol, uint64_t seed, uint64_t first_index,
                 int64_t *sweeps1, int64_t *sweeps2, int64_t *visits2, int64_t *accepted2, uint8_t *ran_phase2, double *f0,
                 double *maxviol);
// for qcqpmi_set_quad and qcqpmi_finalize (launches on c->stream, no wait): the row-major n x n matrix of function k >= 1 in
// c->dn_tmp -> its place in the packed array gpack (dense_pack_kernel); function k of a generator -> row-major padded P
// (dense_gen_rowmajor_kernel); every matrix packed and the vectors of the dense path uploaded (gq, gr, grel: the constraints')
void launch_dense_pack_staged(qcqpmi_ctx *c, int64_t k, double *gpack);
void launch_dense_gen_rowmajor(qcqpmi_ctx *c, double *P, int k, uint64_t seed, double scale, double diag_add);
int dense_build(qcqpmi_ctx *c, const std::vector<double> &gq, const std::vector<double> &gr, const std::vector<int> &grel);
// ONE packed n16 x n16 matrix (the fragment layout of dp.Apack) times the Rpad columns of the tile-major X, 8 row blocks x 8 tiles per
// workgroup (dense_products_kernel<mode>): mode 2: x'Mx per group of row blocks into the dense_product_planes(NB) partial planes
// out[plane][Rpad]; mode 3: out = mu 1' + M X, tile-major
int dense_product_planes(int NB);
int launch_dense_product(qcqpmi_ctx *c, int mode, const double *Mpack, const double *mu, const double *X, double *out);

void admm_drop_handle(qcqpmi_ctx *c);      // capi_admm.hip: the rocBLAS handle of qcqpmi_admm_setup
void comm_drop(qcqpmi_ctx *c);             // capi_comm.hip: the communicator of qcqpmi_comm_init

}  // namespace qcqpmi
