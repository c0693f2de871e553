/*
 * qcqp_mi.h -- C ABI of the MI355X-native Suggest-and-Improve engine (libqcqp_mi.so).
 *
 * This is the drop-in boundary for the hot path of cvxgrp/qcqp.  The reference has no FFI
 * or plugin registry; its seam is the plain-Python call sites
 *     QCQP.suggest            qcqp/qcqp.py:378-401   (RANDOM :381-382, SDR tail :394-401)
 *     QCQP._improve           qcqp/qcqp.py:403-417   (improve_coord_descent :181-192,
 *                                                      improve_admm :254-285)
 * operating on a QCQPForm (qcqp/utilities.py:122-146) of QuadraticFunction objects
 * (qcqp/utilities.py:41-62).  Each entry point below names the reference code it replaces.
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative QCQPMI_E* code and
 *     never throws; qcqpmi_last_error() returns the message for the last failure.
 *   - the caller owns every host buffer (C-contiguous, fp64 / int64) and may free it on return.
 *   - the context owns all device memory and one HIP stream; a context is not thread-safe,
 *     distinct contexts are independent.
 *   - candidate points are handed over as an n x R "column per candidate" array:
 *     candidate r occupies X[r*n .. r*n + n).
 *   - "population" = the device-resident batch of candidates (restarts of improve(), samples of
 *     suggest()); the timed hot path works on the resident population, host copies are explicit.
 *   - relop codes: 0 = none (objective), 1 = '<=', 2 = '=='.
 *   - all arithmetic is fp64.
 */
#ifndef QCQP_MI_H
#define QCQP_MI_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QCQPMI_ABI_VERSION 6

enum {
    QCQPMI_OK = 0,
    QCQPMI_EINVAL = -1,       /* bad argument */
    QCQPMI_EHIP = -2,         /* HIP runtime failure (no device, OOM, launch error) */
    QCQPMI_ESTATE = -3,       /* call order (e.g. run before finalize / without population) */
    QCQPMI_EUNSUPPORTED = -4, /* problem structure not handled by the HIP engine yet */
    QCQPMI_EREFERENCE = -5,   /* the reference would raise on this input (see last_error) */
    QCQPMI_ECOMM = -6         /* RCCL failure */
};

enum { QCQPMI_FMT_DENSE = 0, QCQPMI_FMT_CSR = 1 };

typedef struct qcqpmi_ctx qcqpmi_ctx;

/* ---- library / device ------------------------------------------------------------------ */
int qcqpmi_abi_version(void);
int qcqpmi_device_count(void); /* number of visible HIP devices, 0 if none, never fails */
const char *qcqpmi_last_error(const qcqpmi_ctx *ctx); /* ctx may be NULL: last create error */

/* ---- context = one QCQPForm on one GPU  (utilities.py:122-130) ------------------------- */
int qcqpmi_ctx_create(qcqpmi_ctx **out, int64_t n, int64_t m, int device);
void qcqpmi_ctx_destroy(qcqpmi_ctx *ctx);

/* QuadraticFunction(P, q, r, relop)  (utilities.py:41-46).  k = 0 is the objective f0,
 * k = 1..m the constraints fs[k-1].  P must be symmetric (get_qcqp_form symmetrises,
 * utilities.py:333,345).  DENSE: vals = n*n row-major, idx = ptr = NULL, nnz ignored.
 * CSR: ptr[n+1], idx[nnz], vals[nnz].
 * Constraints that couple coordinates are kept row-major on the device as long as all of them fit 16 GB (the paths in the
 * reference's arithmetic and the device-side ADMM setup read them there); beyond that -- BASELINE.json configs[4] is 137 GB --
 * every coupled function is packed for the matrix cores when this call receives it (streaming upload: no second copy on
 * the host or the device; up to 200 GB of packed matrices) and the problem runs on the dense path only. */
int qcqpmi_set_quad(qcqpmi_ctx *ctx, int64_t k, int format, const double *vals,
                    const int64_t *idx, const int64_t *ptr, int64_t nnz, const double *q,
                    double r, int relop);
/* Synthetic dense function generated ON THE DEVICE, in place of qcqpmi_set_quad for function k
 * (BASELINE.json configs[4]: 1025 dense 4096 x 4096 matrices = 137.6 GB never exist on the host;
 * SURVEY.md section 8(d) cfg5 "generate on device with Philox from the seed"):
 *     P_k[i][j] = scale * w_ij * N(seed, k, min(i,j) n + max(i,j)) + diag_add * [i == j],
 *     w_ii = 1, w_ij = 1/sqrt(2)            (the law of (G + G^T)/2 with G_ij ~ N(0,1), symmetric)
 *     q_k[j]    = qscale * N'(seed, k, j)
 * N, N' = the engine's keyed Philox normal (the generator of qcqpmi_pop_randn; oracle:
 * orc_keyed_normal(seed, 2^48 + k, elem) and orc_keyed_normal(seed, 2^49 + k, j)). */
int qcqpmi_set_quad_generated(qcqpmi_ctx *ctx, int64_t k, uint64_t seed, double scale, double qscale,
                              double diag_add, double r, int relop);
/* Build the device layouts (MFMA-packed P0, per-coordinate constraint lists). */
int qcqpmi_finalize(qcqpmi_ctx *ctx);
/* 1 if every constraint touches exactly one coordinate (Boolean / box families) */
int qcqpmi_is_separable(const qcqpmi_ctx *ctx);

/* ---- population ------------------------------------------------------------------------- */
int qcqpmi_pop_upload(qcqpmi_ctx *ctx, const double *X, int64_t R);
int qcqpmi_pop_download(qcqpmi_ctx *ctx, double *X, int64_t R);
int64_t qcqpmi_pop_size(const qcqpmi_ctx *ctx);
/* suggest(RANDOM) batched: x_r = randn(n)  (qcqp.py:381-382).  Counter-based stream keyed on
 * (seed, first_index + r, element): independent of the sharding over GPUs. */
int qcqpmi_pop_randn(qcqpmi_ctx *ctx, int64_t R, uint64_t seed, uint64_t first_index);
/* suggest(SDR) tail batched: x_s = mu + F xi_s, xi_s ~ N(0, I)  (qcqp.py:396), where
 * F (n x n row-major) is any factor with F F^T = Sigma (the host computes it once: Cholesky, or
 * the SVD factor NumPy's multivariate_normal uses).  Xi (n x S, column per sample) may be given
 * for reproducibility tests; NULL = device Philox normals keyed on (seed, first_index + s).
 * mu == NULL and F == NULL: draw again from the pair of the previous call, which is still resident and packed (no
 * upload; many batches from one relaxation).  Returns without synchronising: the samples are in stream order. */
int qcqpmi_pop_sdr_sample(qcqpmi_ctx *ctx, const double *mu, const double *F, int64_t S,
                          uint64_t seed, uint64_t first_index, const double *Xi);

/* ---- evaluation: QuadraticFunction.eval / violation, QCQPForm.violations
 *      (utilities.py:49-62, 133-134; callers qcqp.py:399-401, 415-417) -------------------- */
/* on the resident population; f0/maxviol have R entries; F (optional) is (m+1) x R row-major */
int qcqpmi_pop_eval(qcqpmi_ctx *ctx, double *f0, double *maxviol, double *F);
/* suggest(SDR) for S samples in ONE call -- draw and evaluate (qcqp.py:396, 399, 401; SURVEY.md section 8b's
 * qcqpmi_sdr_sample_eval): x_s = mu + F xi_s with device Philox normals keyed on (seed, first_index + s), f0[s] = f0(x_s),
 * maxviol[s] = max_k violation_k(x_s).  Chunks of samples are drawn and evaluated back to back in two buffers that every chunk
 * reuses (<= 32 MB each): no population of S points is laid out in HBM.  X_opt (n x S, column per sample, or NULL): the points;
 * with NULL they are not kept -- re-draw the winner from its index (S = 1, first_index + s).  mu == F == NULL: the pair of the
 * previous call.  Afterwards the resident population is the last chunk.  Synchronises before it returns. */
int qcqpmi_sdr_sample_eval(qcqpmi_ctx *ctx, const double *mu, const double *F, int64_t S, uint64_t seed,
                           uint64_t first_index, double *X_opt, double *f0, double *maxviol);
/* host convenience: upload X, evaluate */
int qcqpmi_eval_batch(qcqpmi_ctx *ctx, const double *X, int64_t S, double *f0, double *maxviol,
                      double *F);

/* ---- improve(COORD_DESCENT) on the resident population
 *      (improve_coord_descent qcqp.py:181-192; phase 1 :101-148; phase 2 :152-178;
 *       onevar_qcqp utilities.py:241-288; get_feasible_intervals utilities.py:198-232).
 * Outputs (each R entries, any may be NULL):
 *   sweeps1/sweeps2   sweeps started in phase 1 / phase 2
 *   visits2           coordinate visits of phase 2 (loop bodies of qcqp.py:162)
 *   accepted2         accepted coordinate updates of phase 2
 *   ran_phase2        1 if the restart passed the max-violation gate (qcqp.py:189)
 *   f0/maxviol        objective / max violation of the final point (qcqp.py:415-417)       */
int qcqpmi_cd_run(qcqpmi_ctx *ctx, int phase1, int64_t num_iters, double viol_tol, double tol,
                  uint64_t seed, uint64_t first_index, int64_t *sweeps1, int64_t *sweeps2,
                  int64_t *visits2, int64_t *accepted2, uint8_t *ran_phase2, double *f0,
                  double *maxviol);
/* The same run in stages, for callers that keep two contexts (two HIP streams) on one GPU and overlap the preparation of
 * the next population -- suggest, phase 1, evaluation, gate -- with the phase-2 kernel of the current one, whose tail leaves
 * most CUs idle (bench.py).  stage 0 = qcqpmi_cd_run; 1 = phase 1 + evaluation + gate, asynchronous; 2 = launch of phase 2,
 * asynchronous; 3 = results, blocking.  Stages 1..3 must be called in order with the same parameters; the output pointers
 * are only used by stage 3 (and 0). */
int qcqpmi_cd_run_stage(qcqpmi_ctx *ctx, int stage, int phase1, int64_t num_iters, double viol_tol, double tol,
                        uint64_t seed, uint64_t first_index, int64_t *sweeps1, int64_t *sweeps2,
                        int64_t *visits2, int64_t *accepted2, uint8_t *ran_phase2, double *f0,
                        double *maxviol);
/* Per-restart status codes of the last qcqpmi_cd_run (R ints each; 0 = fine).  A restart on which the
 * reference would raise -- -1: np.random.uniform on an unbounded interval (utilities.py:267), -2: NameError in
 * OneVarQuadraticFunction.eval (utilities.py:119), -3: max() of an empty list (qcqp.py:117), -4: feasible set
 * with more segments than the kernel holds -- is reported here, its f0 / maxviol are +inf (it never wins
 * qcqpmi_select_best) and the other restarts are unaffected.  qcqpmi_cd_run itself returns
 * QCQPMI_EREFERENCE / QCQPMI_EUNSUPPORTED only when EVERY restart failed (R = 1: the reference's behaviour). */
int qcqpmi_cd_status(qcqpmi_ctx *ctx, int *status1, int *status2);

/* ---- unit operators: the reference's module-level helpers for a batch of independent cases, evaluated on the
 * device by the same code the coordinate-descent kernels inline (no context needed).
 *   get_feasible_intervals(f, s)  utilities.py:198-232:  pqrs = count x (p, q, r, s), relop per case;
 *        out = count x (n, lo0, hi0, lo1, hi1), at most two intervals (+-inf as IEEE infinities).
 *   onevar_qcqp(f0, fs, s)        utilities.py:241-288:  f0 = count x (p, q, r); fs = count x 4 x (p, q, r, relop as a
 *        number); nf[i] <= 4 constraints in use; status 1 = a point in x[i], 0 = None, < 0 = the reference raises
 *        (-1 OverflowError in np.random.uniform, -2 NameError in OneVarQuadraticFunction.eval); ties and the
 *        zero-objective draw (utilities.py:266-267, 288) use the keyed Philox stream (seed; case index).
 *        C_out (optional) = count x 5 x (lo, hi): the feasible set after the end-point sweep, nC_out its size. */
int qcqpmi_feasible_intervals_batch(int device, int64_t count, const double *pqrs, const int *relop, double *out);
/*   QuadraticFunction.get_onevar_func(x, k)  utilities.py:99-105: for every function j = 0..m of the problem (objective
 *        first) and every restart r of the resident population, the coefficients of f_j as a function of the coordinate
 *        coord[r] alone: out[(r (m + 1) + j) 3 + (0, 1, 2)] = (t2, t1, t0) = (P[k,k], 2 P[k,:] z + q[k], f_j(z)) with z = x_r,
 *        z[k] = 0, summed in the reference's order by the device functions the coupled-constraint kernel inlines
 *        (csrc/cd_general.h).  Needs the row-major matrices (not device-generated / streamed problems). */
int qcqpmi_onevar_coeffs(qcqpmi_ctx *ctx, const int64_t *coord, double *out);
int qcqpmi_onevar_qcqp_batch(int device, int64_t count, const double *f0, const double *fs, const int *nf,
                             const double *s, uint64_t seed, double *x, int *status, double *C_out, int *nC_out);
/*   The same onevar_qcqp by each instantiation of the set builder + minimiser that a coordinate-descent kernel runs, and one
 *   phase-1 coordinate visit (qcqp.py:113-136) by each of its restatements.  Layouts, draws and status codes as above.
 *        onevar variant: 0 / 1 / 2 = the end-point sweep with 4 / 2 / 1 constraint slots (0 is qcqpmi_onevar_qcqp_batch);
 *            3 / 4 / 5 = the closed form for exactly one constraint, held in 4 / 2 / 1 slots.  C_out keeps 5 pieces per case;
 *            those a variant cannot hold are NaN.
 *        visit variant: 0 / 1 = the generic visit with 1 / 4 slots; 2 = the band class (one constraint p x^2 + r == 0, p > 1e-4)
 *            resolved by hand; 3 / 4 = two band visits fused (r < -1e-3; a case shares the visit with its neighbour i ^ 1 where
 *            that one has the same (p, r), else with a padding element), 4 with the fast first phase of the bisection.
 *            cons = count x 4 x (p, q, r, relop as a number); xi = the coordinate's value before the visit; draws are keyed
 *            (seed; restart = case index; coordinate 0; sweep).  x_out = the value after the visit, moved = 1 where the update was
 *            accepted, vafter = the coordinate's largest violation afterwards, status as qcqpmi_cd_status.
 *   QCQPMI_EINVAL for an unknown variant; QCQPMI_EUNSUPPORTED, before anything is launched, for a case outside the variant's
 *   contract (more constraints than slots, the closed form with nf != 1, a band variant on another constraint or r >= -1e-3). */
int qcqpmi_onevar_variant_batch(int device, int variant, int64_t count, const double *f0, const double *fs, const int *nf,
                                const double *s, uint64_t seed, double *x, int *status, double *C_out, int *nC_out);
int qcqpmi_p1_visit_batch(int device, int variant, int64_t count, const double *cons, const int *nf, const double *xi, double tol,
                          double viol_tol, uint64_t seed, int64_t sweep, double *x_out, int *moved, double *vafter, int *status);

/* ---- improve(ADMM) on the resident population (improve_admm qcqp.py:254-285; admm_phase1 :195-212;
 * admm_phase2 :215-251; onecons_qcqp utilities.py:149-196).  The host supplies what the reference
 * obtains from LAPACK / SuperLU: the eigendecomposition of every constraint matrix (lmb: m x n,
 * Q: m x n x n, NumPy eigh layout: Q[k][:, j] = eigenvector j; cached on the context like f.eigh,
 * utilities.py:160-162) and, for phase 2, Minv = (2 (P0 + rho m I))^-1 (n x n) in place of the
 * SuperLU factorisation of qcqp.py:224-227.  rho must already be validated / chosen by the caller
 * (qcqp.py:261-278).  Minv may be NULL when P0 is diagonal (the inverse is formed on the device).  Outputs (R entries
 * each, may be NULL): iterations of phase 1 / phase 2, objective and max violation of the returned points. */
int qcqpmi_admm_set_eig(qcqpmi_ctx *ctx, const double *lmb, const double *Q);
/* The same cache computed ON THE DEVICE (f.eigh = LA.eigh(P), utilities.py:160-162, for every constraint at once:
 * rocSOLVER batched dsyevd on the resident dense matrices) -- for problems whose constraints couple coordinates.
 * Eigenvectors of degenerate eigenvalues span the same spaces as LAPACK's but are a different basis: iterates
 * agree with qcqpmi_admm_set_eig to rounding, not bit for bit. */
int qcqpmi_admm_setup(qcqpmi_ctx *ctx);
/* REDUCED bases for low-rank constraints (beamforming: rank 2).  onecons_qcqp (utilities.py:149-196) moves a point only
 * inside span(B_k), B_k = [eigenvectors of the nonzero eigenvalues of P_k, the unit vector along the part of q_k outside
 * them (eigenvalue 0)]: with lam (m x rp), Bv (m x rp x n, basis vector j of constraint k contiguous, orthonormal, zero
 * padded) and qhat = B_k^T q_k (m x rp) the ADMM iteration runs on (m rp) x n operators instead of (m n) x n --
 * algebraically the same iteration (duals live in span(B_k)).  The multiplier bracket comes from the nonzero
 * eigenvalues given here, not from LAPACK's round-off eigenvalues of the null space: results agree
 * with the full-basis path to the accuracy of the reference's own bisection (1e-6 on every multiplier). */
int qcqpmi_admm_set_basis(qcqpmi_ctx *ctx, int64_t rp, const double *lam, const double *Bv, const double *qhat);
/* Optional: the multiplier bracket [slo_k, ehi_k] (m values each, host) that the bisection of onecons_qcqp starts from
 * (utilities.py:176-186), replacing the one qcqpmi_admm_set_eig / _set_basis / _setup derived from their own eigenvalues;
 * -inf / +inf = "no eigenvalue of that sign": the reference's doubling search from -1 / +1.  The reference brackets with
 * EVERY eigenvalue LAPACK returns, round-off eigenvalues of the null space included (a rank-2 PSD matrix has n - 2
 * eigenvalues ~ +-1e-15, so ehi = -1 / min(lmb) ~ 1e14 instead of the doubling search); with the reference's
 * bracket the reduced-basis path visits the reference's midpoints and returns its multiplier bit for bit instead of
 * "within the bisection tolerance 1e-6".  The parity tests pass the bracket of the eigenvalues they hand the oracle. */
int qcqpmi_admm_set_bracket(qcqpmi_ctx *ctx, const double *slo, const double *ehi);
/* out[k] = P_k Vin_k for every constraint k (n x p blocks, row-major; shared != 0: one Vin for all): the two passes over
 * the resident dense constraint matrices that a randomised range finder needs (Y = P Omega, Z = P Q) -- the device-side
 * part of building the reduced bases above without an O(n^3) eigendecomposition per constraint. */
int qcqpmi_admm_apply_constraints(qcqpmi_ctx *ctx, int p, const double *Vin, int shared, double *out);
/* onecons_qcqp(z, f_k) (utilities.py:149-196) for every resident point z, k = 1..m, with the installed eigenpairs /
 * basis: out = R x n projections (host layout of qcqpmi_pop_download); the population is not changed.  (The reference's
 * own test examples/tests/one_constraint_qcqp.py exercises exactly this function.) */
int qcqpmi_admm_onecons(qcqpmi_ctx *ctx, int64_t k, double *out);
/* Device-side setup of the z-update for a non-diagonal P0: (2 (P0 + rho m I))^-1 -- the matrix the reference factorises
 * with SuperLU (qcqp.py:224-227) -- by a Newton-Schulz iteration on the engine's own GEMM; kept packed inside the context.
 * A following qcqpmi_admm_run with the same rho may then pass Minv = NULL.  resid_out: estimate of max |I - M X| reached;
 * iters_out: iterations taken.  Fails (QCQPMI_EREFERENCE) if P0 + rho m I is not positive definite. */
int qcqpmi_admm_zsolver_device(qcqpmi_ctx *ctx, double rho, int64_t max_iter, double *resid_out, int64_t *iters_out);
/* lambda_min(P0) for the rho check / auto-rho of improve_admm (qcqp.py:262, 272: LA.eigh in the reference): Lanczos with
 * full reorthogonalisation, the products P0 v on the device.  max_steps <= 0: up to n steps. */
int qcqpmi_p0_lambda_min(qcqpmi_ctx *ctx, int64_t max_steps, double tol, double *lmin_out, int64_t *steps_out);
int qcqpmi_admm_run(qcqpmi_ctx *ctx, int phase1, int64_t num_iters, double tol, double viol_lim,
                    double rho, const double *Minv, int64_t *iters1, int64_t *iters2, double *f0,
                    double *maxviol);   /* Minv may be NULL if P0 is diagonal or after qcqpmi_admm_zsolver_device(rho) */
/* With reduced bases (qcqpmi_admm_set_basis, rp <= 8) and a diagonal P0 -- BASELINE.json configs[3] -- qcqpmi_admm_run runs
 * improve_admm (qcqp.py:254-285: phase 1, better, phase 2 with its bestx bookkeeping, better) inside ONE persistent kernel
 * per tile of 16 restarts (csrc/admm_fused.hip; a tile may be shared by a cluster of 2..16 workgroups so that few restarts
 * still fill the chip), no host in the loop.  qcqpmi_admm_fused(ctx, 0) selects the multi-launch path everywhere (the
 * cross-check; same iteration, other summation order in the two products); default 1.  qcqpmi_last_admm_kernel names the
 * path the last run took ("admm_fused_kernel" / "admm_multi_launch") and the workgroups per tile it used.
 * enable == 2 (round 5, experiment kept as a cross-check): the same kernel with FOUR-wave workgroups, two per compute unit,
 * twice as many workgroups per tile -- the co-resident workgroups belong to different tiles; measured equal to the
 * eight-wave geometry at 1024 restarts and slower elsewhere, hence not the default. */
int qcqpmi_admm_fused(qcqpmi_ctx *ctx, int enable);

/* Unit bases (round 5).  When every basis vector handed to qcqpmi_admm_set_basis is +-e_i -- separable constraints
 * p x_i^2 + q x_i + r ~ 0 (Boolean least squares, MAXCUT, boxes; /root/reference/examples/boolean_least_squares.py:34-36,
 * maxcut.py:25-28), for which the eigenvectors utilities.py:160-162 takes from LAPACK are unit vectors -- qcqpmi_admm_run
 * replaces the two consensus products of an iteration (qcqp.py:204-207, 236-239 in the basis) by a gather and a scatter:
 * the same values, no n x m operator.  With one row per constraint the z-update, the gather, the projections
 * (onecons_qcqp, utilities.py:149-196) and the scatter of an iteration are ONE launch (admm_unit_step_kernel; the same bits
 * as the separate launches).  On by default; enable = 0 forces the GEMM path (cross-check). */
int qcqpmi_admm_unit_bases(qcqpmi_ctx *ctx, int enable);
const char *qcqpmi_last_admm_kernel(qcqpmi_ctx *ctx, int *workgroups_per_tile);

/* Y = (sum_k w_k P_k) X for the resident population (w: m+1 weights, objective first; Y: R x n like
 * qcqpmi_pop_download).  Building block of the general SDP-relaxation solver (qcqp_amd/sdr.py: the gradient of
 * the Burer-Monteiro augmented Lagrangian is 2 S V with S = C + sum_k y_k M_k); one streaming pass over all
 * matrices + one GEMM.  For problems whose constraints are separable only the objective has a matrix: Y = w_0 P0 X
 * (the constraints are elementwise operators the caller applies itself). */
int qcqpmi_pop_weighted_product(qcqpmi_ctx *ctx, const double *w, double *Y);
/* S = sum_k w_k P_k itself (n x n row-major on the host): the dual matrix of the SDP certificate when the matrices
 * only exist on the device.  qcqpmi_get_linear returns q_k, r_k, relop of function k as the context holds them
 * (also for device-generated functions). */
int qcqpmi_weighted_matrix(qcqpmi_ctx *ctx, const double *w, double *S);
int qcqpmi_get_linear(qcqpmi_ctx *ctx, int64_t k, double *q, double *r, int *relop);
/* Quadratic and linear parts of every function for the resident population, kept apart:
 * quad[k][r] = x_r' P_k x_r + r_k,  lin[k][r] = q_k' x_r   ((m+1) x R each, row-major).  Same kernels as the
 * evaluation of QuadraticFunction.eval (utilities.py:49-50); the SDP solver needs the parts of the homogeneous forms. */
int qcqpmi_pop_eval_parts(qcqpmi_ctx *ctx, double *quad, double *lin);

/* solve_sdr (qcqp.py:72-97) for the UNIT-DIAGONAL family -- constraints x_i^2 = d_i, i.e. Boolean least
 * squares, MAXCUT, partitioning; the host scales d to 1:
 *     minimise <C, X>  s.t.  X_ii = 1, X PSD,   C symmetric N x N (N = n + 1, homogenised, row-major)
 * in Burer-Monteiro form X = V V^T (V: N x 64, unit rows) by the mixing method on the device.  V holds the
 * start on entry and the solution on return; hist[0] = start objective, hist[t] = objective after sweep
 * t, hist[*sweeps_done + 1] = objective recomputed at the end (hist has max_sweeps + 2 entries).
 * The reference delegates this to cvxpy + an SDP solver: parity unpinned, validated by optimality
 * conditions. */
int qcqpmi_sdr_solve_unitdiag(qcqpmi_ctx *ctx, const double *C, int64_t N, double *V, int max_sweeps,
                              double tol, double *hist, int *sweeps_done);

/* ---- QCQPForm.better ordering over the population (utilities.py:135-146):
 * lexicographic minimum of (int(maxviol/tol), f0), ties -> lowest index.  Evaluates the
 * population if needed.  best_x (n doubles) may be NULL. */
int qcqpmi_select_best(qcqpmi_ctx *ctx, double tol, int64_t *best_index, double *best_f0,
                       double *best_maxviol, double *best_x);

/* ---- timing of the hot kernels (HIP events on the context's stream) ---------------------
 * which: 0 = eval, 1 = cd phase 1, 2 = cd phase 2, 3 = sdr sampling, 4 = admm secular kernel.  Returns the duration of
 * the most recent launch of that kernel in milliseconds. */
int qcqpmi_last_kernel_ms(qcqpmi_ctx *ctx, int which, double *ms);
/* name of the phase-2 kernel the most recent qcqpmi_cd_run dispatched to: "cd_phase2_q_kernel" (pipelined, Boolean family),
 * "cd_phase2_rs_kernel" (its predecessor: box families, n not a multiple of 16, n > 1024), "cd_phase2_kernel" (general
 * separable constraints), "dense_chain_kernel" (constraints that couple coordinates, n > 64 or generated),
 * "cd_general_kernel" (coupled constraints in the reference's arithmetic); static storage.  The parity tests assert it. */
const char *qcqpmi_last_cd_kernel(qcqpmi_ctx *ctx);
/* Scheduling of phase 2 for the Boolean family (the headline kernel).  0: a workgroup is bound to a tile of 16 restarts for
 * the whole launch (cd_phase2_q_kernel: it runs until its slowest restart has converged).  1: a workgroup owns 16 SLOTS; a
 * restart that is done (qcqp.py:172-176, or num_iters sweeps) is written out at the next sweep boundary and its slot takes the
 * next restart from a device-side queue (cd_phase2_qs_kernel, csrc/cd_queue.hip).  Per restart the same arithmetic; results
 * do not depend on the scheduling (every product is summed in one association).  qcqpmi_last_cd_kernel names the kernel. */
int qcqpmi_cd_queue(qcqpmi_ctx *ctx, int mode);     /* 0 off, 1 on wherever it applies, 2 (default) auto: more tiles than CUs */
/* (ABI 4 removed the round-3 experiments around that kernel -- qcqpmi_cd_chain, qcqpmi_cd_partition, qcqpmi_cd_ring_start /
 * submit / collect / stop: launches that ran restarts of other contexts' populations, a CU-masked stream, one persistent
 * spin-waiting launch for several contexts.  They needed GPU_MAX_HW_QUEUES > 4, worked on the 192-CU partition only and could
 * stall; qcqpmi_cd_stream_run below does what they were after inside ONE self-contained launch.) */
/* debug (after qcqpmi_debug_profile enabled profiling): tick sums (s_memtime) over the workgroups of the last
 * qcqpmi_cd_stream_run launch, TWENTY-FOUR entries (ABI 5; 8 before) -- [0] column build (suggest + phase 1 + gate), [1] whole launch,
 * [2] episodes, [3] columns built, [4] the normals' share of [0], [5] the roles of the episodes (the rest: write-out, queue,
 * refill); cd_life_kernel only: [6] workgroups whose waves covered the four SIMDs evenly, [8] the chain waves' wait for
 * partial tiles, [9] / [10] multiplying wave 0's waits for a commit / for its slot, [11] block intervals, [12] blocks with a
 * near-tie replay, [13] / [14] / [15] / [7] the chain's stages: sum of the partial tiles + requests, the 16 steps, block end +
 * commit, fix-up + own share + staging, [16] the longest workgroup's [1] (ticks of the launch as the device saw it: with the
 * HIP-event duration the tick rate; [1] / workgroups / [16] = how much of the launch the average workgroup was alive), [17] column
 * build up to the end of phase 1, [18] the chain's prologue per episode (virtual interval, operands of block 0), [19] issuing an
 * interval's memory requests (top of the chain's loop: not part of [13]), [20] from the chain's last interval to the barrier
 * that ends the episode */
int qcqpmi_debug_life_profile(qcqpmi_ctx *ctx, int64_t *out24);
/* POPULATION STREAMING (round 4) -- the reference's user loop `for ...: suggest(); improve(COORD_DESCENT)` (README.md:51-57)
 * for K populations of R restarts in ONE persistent launch: a workgroup owns 16 restart slots; a slot that becomes free draws
 * the next restart index of the run and runs that restart's WHOLE step itself -- suggest(RANDOM) (qcqp.py:381-382; the keyed
 * normals of qcqpmi_pop_randn), phase 1 (qcqp.py:101-149), the gate (qcqp.py:189), phase 2 to convergence (qcqp.py:152-178),
 * objective and max violation of the result -- so the matrix pipes work on live restarts across population boundaries and no
 * preparation kernel, second stream or CU partition exists (csrc/cd_queue.hip, lifecycle mode).  Population p uses the seed
 * seed + p seed_stride and the global restart indices first_index + p first_stride + [0, R): every restart equals the one
 * qcqpmi_pop_randn(R, seed_p, first_p) + qcqpmi_cd_run would produce (same draws, same moves; the reported objective is a fresh
 * evaluation of the final point summed from the products of the restart's last sweep instead of the tracked value: 1e-12
 * relative).  generate = 0: the K R resident points (qcqpmi_pop_upload) are the starts instead of normals.  Outputs: per-restart
 * arrays of K R entries (population-major; may be NULL) as in qcqpmi_cd_run, and per population the best restart (index within
 * the population, QCQPForm.better ordering with bucket width select_tol), its objective, max violation and point (K x n).
 * The K R final points stay resident (qcqpmi_pop_download).
 * Round 5 (ABI 5): the launch is cd_life_kernel (csrc/cd_life.hip) -- four-wave workgroups, two per CU, the X tile in a private
 * global tile instead of LDS -- and takes every problem with separable constraints of ONE class, one constraint per coordinate
 * (Boolean / MAXCUT x_i^2 == 1, box and disc x_i^2 <= c, one-sided and linear single-coordinate constraints), a diagonal of P0
 * that is positive everywhere or ZERO everywhere (MAXCUT: qcqp.py:152-178 with a linear scalar objective), any 48 <= n <= 2304
 * (n need not be a multiple of 16; 1024 < n <= 2304 runs eight-wave workgroups).  Round 6 (ABI 6): ALSO problems with up to four
 * classes of coordinates (coordinates whose constraint lists are bit-identical share a class) and up to two constraints per
 * coordinate -- boxes with different bounds, an annulus beside an equality, two linear bounds, MAXCUT with relaxed vertices
 * (qcqp.py:113-141, 160-176 treat every coordinate's list on its own); ONE lifecycle kernel for every shape; with
 * qcqpmi_cd_set_objective_factor the kernel carries L^T X instead of multiplying with P0 and takes n up to 4096.
 * Round 7: ALSO a diagonal of P0 of MIXED sign -- negative entries, or zero in some places and not in others: a box-constrained QP
 * with an indefinite P0 -- for ONE class with one constraint per coordinate and a bounded feasible set of one or two intervals,
 * 33 <= n <= 2304, no objective factor (qcqpmi_last_cd_kernel: "cd_life_kernel<3,sgn>" / "cd_life_kernel<7,sgn>"): every coordinate
 * steps by the sign of its own P0[i,i] (utilities.py:262-288: the vertex if P0[i,i] > 0 and it is feasible, else the best end point).
 * QCQPMI_EUNSUPPORTED otherwise (more than four classes, three or four constraints per coordinate, mixed diagonal signs together
 * with several classes or two constraints per coordinate, coupled constraints, n > 2304 without an objective factor): use
 * qcqpmi_cd_run per population; a refused call leaves the resident population untouched.  K R < 2^30 (restart tickets are 32-bit; QCQPMI_EINVAL beyond).
 * Near-ties: a restart whose decision is within rounding of a tie is replayed in the reference's arithmetic like in
 * qcqpmi_cd_run; for a positive diagonal the replay sees the objective RELATIVE to the start of phase 2 (the constant of its
 * scalar objective differs from the reference's by f0 at that start: candidates closer than one ulp of f0 may resolve
 * differently; exact ties do not), for a zero diagonal the absolute objective (evaluated by an extra frozen sweep).  A diagonal of
 * mixed sign tracks the ABSOLUTE objective like the zero diagonal (the same extra frozen sweep per restart): wherever P0[i,i] <= 0
 * the reference compares rounded absolute values f0(end point), and a replay that saw a relative objective could resolve candidates
 * within one ulp of f0 differently there; its coordinates with P0[i,i] > 0 see the absolute value too, i.e. the reference's own
 * constant.  A decision counts as a near-tie when the vertex of a coordinate with P0[i,i] > 0 is within 1e-7 of the gap from the
 * gap's midpoint (as for a positive diagonal), or when the two outermost end points' values differ by less than 1e-12 of the
 * objective's scale (sum |P0| + sum |q0| + |r0|, times the largest squared end point if above 1) times the ratio of their distance
 * to the narrower interval's width, for P0[i,i] <= 0 (as for a zero diagonal, the secant slope in place of the slope). */
int qcqpmi_cd_stream_run(qcqpmi_ctx *ctx, int64_t K, int64_t R, int generate, int phase1, int64_t num_iters, double viol_tol,
                         double tol, uint64_t seed, uint64_t seed_stride, uint64_t first_index, uint64_t first_stride,
                         double select_tol, int64_t *sweeps1, int64_t *sweeps2, int64_t *visits2, int64_t *accepted2,
                         uint8_t *ran_phase2, double *f0, double *maxviol, int64_t *best_index, double *best_f0,
                         double *best_maxviol, double *best_x);
/* MANY SMALL PROBLEMS IN ONE LAUNCH (added within ABI 6: a new symbol, nothing else changes).  B problems that share n <= 64
 * and ONE set of separable constraint lists -- those of this context, created and finalized as usual with any objective as
 * function 0 (every class and up to four constraints per coordinate, as qcqpmi_cd_run takes them) -- and differ in their objective:
 * P0s [B][n][n] (each symmetric, any diagonal sign, any definiteness), q0s [B][n], r0s [B].  A frame of MIMO detection problems is
 * the example: thousands of Boolean least squares instances with n = 8 .. 64, P0_b = A_b^T A_b, q0_b = -2 A_b^T b_b, x_i^2 == 1.
 * Every problem gets R restarts.  Restart (b, r) IS the restart r that a context holding the constraints and objective b produces by
 *     qcqpmi_pop_randn(R, seed + b seed_stride, first_index)        (generate = 0: the uploaded starts X0 [B][R][n] instead)
 *     qcqpmi_cd_run(phase1, num_iters, viol_tol, tol, seed + b seed_stride, first_index):
 * the same keyed draws by the global restart index first_index + r (normals, tie draws, the zero-objective draw), the same phase 1,
 * gate, phase 2, counters and status codes; the moves agree to the rounding of the row sums (P0 x)_i (summed in index order here, on
 * the matrix cores there).  A result depends on (objective b, its seed, the global index) alone: not on B, not on the problems
 * beside b, not on the number of workgroups or the order in which the work is dealt out -- bit for bit.
 * One persistent launch of cd_small_kernel (csrc/cd_small.hip): one wavefront per (problem, restart), lane = coordinate, P0_b staged
 * in LDS once per workgroup.  Outputs, any may be NULL: per restart [B R] (problem-major) the arrays of qcqpmi_cd_run, the status
 * codes of qcqpmi_cd_status (a restart with a code != 0 reports f0 = maxviol = +inf and never wins; the call itself succeeds) and the
 * final points X [B][R][n]; per problem [B] the best restart (index within the problem; QCQPForm.better ordering with bucket width
 * select_tol, ties -> lowest index, like qcqpmi_select_best), its objective, max violation and point best_x [B][n].
 * QCQPMI_EUNSUPPORTED: constraints that are not separable, n > 64.  QCQPMI_EINVAL: B < 1, R < 1, B R >= 2^30, a missing input, a
 * P0_b that is not symmetric.  The call works in buffers of its own: the resident population, its evaluation and its status codes
 * stay as they were, whether the call succeeds or is refused.  qcqpmi_last_cd_kernel: "cd_small_kernel<1>" (at most one constraint
 * per coordinate) / "cd_small_kernel<4>". */
int qcqpmi_cd_small_batch_run(qcqpmi_ctx *ctx, int64_t B, const double *P0s, const double *q0s, const double *r0s, int64_t R,
                              int generate, const double *X0, int phase1, int64_t num_iters, double viol_tol, double tol,
                              uint64_t seed, uint64_t seed_stride, uint64_t first_index, double select_tol, int64_t *sweeps1,
                              int64_t *sweeps2, int64_t *visits2, int64_t *accepted2, uint8_t *ran_phase2, int *status1,
                              int *status2, double *f0, double *maxviol, double *X, int64_t *best_index, double *best_f0,
                              double *best_maxviol, double *best_x);
/* THE SAME LAUNCH WITH PER-PROBLEM CONSTRAINT COEFFICIENTS (added within ABI 6: a new symbol, nothing else changes).  The context
 * fixes the STRUCTURE of the constraints -- their number m, the coordinate constraint k touches and its relop -- and every problem
 * brings its own coefficients: cons [B][m][3], (p, q, r) of constraint k of problem b at cons[(b m + k) 3 ..], k = 0..m-1 in the
 * order of qcqpmi_set_quad (k + 1 there); p is the diagonal entry P_k[i,i] and q the linear entry q_k[i] on the coordinate i that
 * constraint k touches in the context, r the constant: the values qcqpmi_finalize keeps per list entry.  Box-constrained QPs with
 * bounds per instance ((x_i - lo)(x_i - hi) <= 0: p = 1, q = -(lo + hi), r = lo hi), annuli with per-instance radii, x_i^2 == d_{b,i}.
 * PARITY.  Restart (b, r) is BIT FOR BIT restart r of qcqpmi_cd_small_batch_run called with B = 1 and seed + b seed_stride on a
 * context created from problem b's own functions (same structure, b's coefficients); that restart is in turn the qcqpmi_pop_randn +
 * qcqpmi_cd_run restart of that context, to the rounding stated above.  A result depends on (objective b, constraints b, seed of b,
 * global index) alone.  A call whose cons repeats the context's coefficients for every problem equals the shared call bit for bit.
 * The ticket's workgroup stages problem b's coefficients in LDS beside P0_b (cd_small_kernel<MAXC, pc>: 24 m bytes more, at most
 * 6 KB); qcqpmi_last_cd_kernel: "cd_small_kernel<1,pc>" / "cd_small_kernel<4,pc>".  Refusals, the resident population left alone:
 * those of qcqpmi_cd_small_batch_run, and QCQPMI_EINVAL for cons == NULL, a coefficient that is not finite, or a constraint of some
 * problem with p == 0 and q == 0 (it touches no coordinate: no context could have been built from it). */
int qcqpmi_cd_small_batch_run_pc(qcqpmi_ctx *ctx, int64_t B, const double *P0s, const double *q0s, const double *r0s,
                                 const double *cons, int64_t R, int generate, const double *X0, int phase1, int64_t num_iters,
                                 double viol_tol, double tol, uint64_t seed, uint64_t seed_stride, uint64_t first_index,
                                 double select_tol, int64_t *sweeps1, int64_t *sweeps2, int64_t *visits2, int64_t *accepted2,
                                 uint8_t *ran_phase2, int *status1, int *status2, double *f0, double *maxviol, double *X,
                                 int64_t *best_index, double *best_f0, double *best_maxviol, double *best_x);
/* THE BATCH FOR PROBLEMS OF UP TO 128 VARIABLES (added within ABI 6: a new symbol, nothing else changes).  The arguments of
 * qcqpmi_cd_small_batch_run_pc; cons may be NULL: shared constraints, the context's.  1 <= n <= 128.
 * n <= 64: exactly the launch of qcqpmi_cd_small_batch_run (cons == NULL) or qcqpmi_cd_small_batch_run_pc -- the same kernel, the same
 * bits, the same name in qcqpmi_last_cd_kernel.
 * 65 <= n <= 128: the WIDE kernels cd_small_kernel<MAXC, pc, 2> -- one wavefront per (problem, restart) as before, lane l holds the
 * coordinates l and l + 64 (the second one where l + 64 < n); a visit of coordinate i reads slot i >> 6 at lane i & 63 and its rank-one
 * update covers both slots.  The LDS image is the same -- P0_b row-major n x n, q0_b, the [3][m] coefficients with cons, two control
 * words: (n^2 + n + 3 m) 8 + 8 bytes, at most 144 392 of the 160 KB of a CU; from n = 101 one workgroup (512 threads, eight waves)
 * owns a CU.  A 64 x 64 QPSK MIMO frame (128 real variables) is the example.
 * PARITY: that of the two symbols above, unchanged.  Every sum is formed in the same order (row sums over k ascending, the objective
 * over j ascending across both slots), the keyed draws go by the coordinate index, status1 is that of the highest coordinate with a
 * nonzero code.  A result depends on (objective b, constraints b, seed of b, global index) alone -- not on B, the neighbours, the order
 * of the problems, the workgroups or a split of the restarts over calls: bit for bit.  With cons, restart (b, r) is bit for bit the
 * restart of the call with B = 1, cons == NULL on a context created from problem b's own functions.
 * qcqpmi_last_cd_kernel for n > 64: "cd_small_kernel<1,w2>" / "<4,w2>" / "<1,pc,w2>" / "<4,pc,w2>".
 * Refusals, the resident population left alone.  QCQPMI_EUNSUPPORTED: n > 128, constraints that are not separable.  QCQPMI_EINVAL:
 * B < 1, R < 1, B R >= 2^30, a missing array, a cons entry that is not finite or has p == q == 0, a P0_b that is not symmetric. */
int qcqpmi_cd_batch_run(qcqpmi_ctx *ctx, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *cons,
                        int64_t R, int generate, const double *X0, int phase1, int64_t num_iters, double viol_tol, double tol,
                        uint64_t seed, uint64_t seed_stride, uint64_t first_index, double select_tol, int64_t *sweeps1,
                        int64_t *sweeps2, int64_t *visits2, int64_t *accepted2, uint8_t *ran_phase2, int *status1, int *status2,
                        double *f0, double *maxviol, double *X, int64_t *best_index, double *best_f0, double *best_maxviol,
                        double *best_x);
/* SUGGEST(SDR) FOR MANY SMALL PROBLEMS IN ONE LAUNCH (added within ABI 6: a new symbol, nothing else changes).  The batch of
 * qcqpmi_cd_small_batch_run -- B objectives P0s [B][n][n] (each symmetric), q0s [B][n], r0s [B] over this context's constraints, n <= 64
 * -- for the UNIT-DIAGONAL family: every coordinate carries exactly one constraint p x_i^2 + r == 0 with d_i = -r / p > 0 and no linear
 * term (Boolean least squares, MAXCUT, x_i^2 == d_i).  With N = n + 1 and s = sqrt(d), problem b's relaxation is
 *     minimise <C_b, X>  s.t.  X_ii = 1, X PSD,   C_b[:n,:n] = P0_b o s s^T, C_b[:n,n] = C_b[n,:n] = q0_b o s / 2, C_b[n,n] = r0_b,
 * solved in the form X = V V^T (V: N x 64, unit rows) by the mixing method of qcqpmi_sdr_solve_unitdiag (cyclic updates, the sweep
 * objective tracked by the exact decrease of every update, stop at |delta_sweep| <= tol (1 + |f|) or max_sweeps, a row whose g_i is
 * zero stays as it is) -- one wavefront per problem, V_b and C_b in its LDS, no wave waits for another (sdr_small_kernel,
 * csrc/sdr_small.hip).  The same launch forms the multipliers y_i = -v_i . (C_b v)_i and draws S >= 0 samples per problem,
 *     x = s o (V_n u + V_n (xi - u (u . xi))),   u = v_n,  V_n = rows 0..n-1,  xi_k = keyed normal (seed_b, first_index + sigma, k), k < 64:
 * x ~ N(mu, Sigma) with mu = s o V_n u and Sigma = F F^T, F = diag(s) V_n (I - u u^T) -- the pair of suggest(SDR) (qcqp.py:394-396)
 * without a decomposition (I - u u^T is a projector).  seed_b = seed + b seed_stride.  Start: row i of V0 = the keyed normals
 * (seed_b, 2^64 - 1 - i, k), k < 64, divided by the root of their sum of squares (summed as a binary tree over adjacent k); or V0s
 * [B][N][64], taken as it is.  The reference hands the relaxation to a third-party solver: parity unpinned by construction, validated
 * by the certificate (lambda_min(C_b + diag(y_b)), qcqp_amd.sdr.certify_batch).  A problem's result depends on (P0_b, q0_b, r0_b, d,
 * seed_b, first_index) alone -- not on B, the problems beside it, the workgroups or the dealing order: bit for bit.
 * Outputs, any may be NULL: V [B][N][64], primal [B] (<C_b, V V^T> recomputed at the end), y [B][N], sweeps [B], X [B][S][n].
 * QCQPMI_EUNSUPPORTED: constraints outside the family, n > 64.  QCQPMI_EINVAL: B < 1, S < 0, B S >= 2^30, a missing input, a P0_b that is
 * not symmetric.  The call works in a buffer of its own: the resident population, its evaluation, its status codes and
 * qcqpmi_last_cd_kernel stay as they were, whether the call succeeds or is refused. */
int qcqpmi_sdr_small_batch(qcqpmi_ctx *ctx, int64_t B, const double *P0s, const double *q0s, const double *r0s, int64_t S,
                           int max_sweeps, double tol, uint64_t seed, uint64_t seed_stride, uint64_t first_index,
                           const double *V0s, double *V, double *primal, double *y, int64_t *sweeps, double *X);
/* THE SAME LAUNCH WITH PER-PROBLEM d (added within ABI 6: a new symbol, nothing else changes): problem b has the constraints
 * x_i^2 == ds[b n + i], ds [B][n], every entry > 0 and finite; the context must be of the unit-diagonal family as above and ds
 * replaces its d problem by problem (s_b = sqrt(ds_b) scales C_b and the samples).  PARITY: problem b's V, y, primal, sweeps and X are
 * BIT FOR BIT those of qcqpmi_sdr_small_batch called with B = 1 and seed + b seed_stride on a context created from problem b's own
 * functions (d = ds_b); a result depends on (objective b, ds_b, seed of b, first_index) alone.  Refusals: those of
 * qcqpmi_sdr_small_batch, and QCQPMI_EINVAL for ds == NULL or an entry that is not positive and finite. */
int qcqpmi_sdr_small_batch_pc(qcqpmi_ctx *ctx, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *ds,
                              int64_t S, int max_sweeps, double tol, uint64_t seed, uint64_t seed_stride, uint64_t first_index,
                              const double *V0s, double *V, double *primal, double *y, int64_t *sweeps, double *X);
/* THE SAME TWO CALLS FOR 1 <= n <= 128 (added within ABI 6: two new symbols, nothing else changes).  The arguments, outputs and
 * refusals are those of qcqpmi_sdr_small_batch and qcqpmi_sdr_small_batch_pc.  For n <= 64 they make exactly that launch: bit for bit
 * the same results.  For 65 <= n <= 128 the wide kernel runs (sdr_small_kernel<true>, csrc/sdr_small.h): still one wavefront per
 * problem, rank 64, the same start, passes, stop rule and sums in the same order, with C_b stored as its lower triangle (N (N + 1) / 2
 * doubles: the LDS image is 134 672 bytes at n = 128, one wavefront per CU) and two coordinates per lane in the samples (lane l forms
 * x_l and x_{l+64}).  V0s and V stay [B][N][64].  The bit-for-bit statements above hold as they stand.  QCQPMI_EUNSUPPORTED: n > 128,
 * constraints outside the family.  The old symbols refuse n > 64 as before. */
int qcqpmi_sdr_batch(qcqpmi_ctx *ctx, int64_t B, const double *P0s, const double *q0s, const double *r0s, int64_t S, int max_sweeps,
                     double tol, uint64_t seed, uint64_t seed_stride, uint64_t first_index, const double *V0s, double *V,
                     double *primal, double *y, int64_t *sweeps, double *X);
int qcqpmi_sdr_batch_pc(qcqpmi_ctx *ctx, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *ds,
                        int64_t S, int max_sweeps, double tol, uint64_t seed, uint64_t seed_stride, uint64_t first_index,
                        const double *V0s, double *V, double *primal, double *y, int64_t *sweeps, double *X);
/* SUGGEST(SPECTRAL) FOR MANY SMALL PROBLEMS IN ONE LAUNCH (added within ABI 6: a new symbol, nothing else changes).  B objectives
 * P0s [B][n][n] (each symmetric), q0s [B][n], r0s [B], 1 <= n <= 64, whose constraints ALL carry one relop (relop_eq != 0: ==, else <=)
 * and, summed as suggest(SPECTRAL) sums them (qcqp.py:41-70), give ONE constraint
 *     c(x) = sum_i (a_i x_i^2 + beta_i x_i) + gamma  (relop)  0,   every a_i > 0,   rho^2 = sum_i beta_i^2 / (4 a_i) - gamma > 0:
 * agg = [a (n) | beta (n) | gamma], one for all problems (agg_stride = 0) or [B][2 n + 1] (agg_stride = 2 n + 1).  The context
 * supplies n, the device and its buffers; its own constraints are not read.  The reference's relaxation
 *     minimise <W0, X>  s.t.  <Wc, X> (relop) 0,  X_NN = 1,  X PSD
 * has one quadratic constraint, so it is exact and its value is that of  min f0(x) s.t. c(x) (relop) 0 -- a trust-region problem
 * on a sphere or ball.  With s = sqrt(a), y = s o x + beta / (2 s):  c = |y|^2 - rho^2,  f0 = y'Ay + 2 g'y + const,  A = S^-1 P0 S^-1.
 * One wavefront per problem (spectral_small_kernel, csrc/spectral_small.hip), A_b and Q_b in its LDS, no wave waits for another:
 * A = Q diag(lam) Q' by cyclic two-sided Jacobi in a fixed round-robin order (csrc/jacobi_small.h; stop at off(A) <= tol |A|_F or
 * max_sweeps), then in the lanes the multiplier mu >= -lam_min (and >= 0 for <=) with sum_k gh_k^2 / (lam_k + mu)^2 = rho^2,
 * gh = Q'g, by a safeguarded Newton iteration with a fixed rule, and y = -Q (gh / (lam + mu)); for <= with lam_min > 0 and the
 * unconstrained minimiser in the ball mu = 0; in the hard case (g without a component in the lowest eigenspace, the rest shorter
 * than rho; threshold 2^-46, csrc/spectral_solve.h) mu = -lam_min and y = y_reg + tau q_min, tau >= 0, q_min with its entry of
 * largest magnitude positive.  Every wave sum has one order: a problem's result depends on (P0_b, q0_b, r0_b, agg_b, relop_eq,
 * max_sweeps, tol) alone -- not on B, the problems beside it, the workgroups or the dealing order: bit for bit.  The reference
 * hands the relaxation to a third-party solver and reads its point off an eigenvector of arbitrary sign: parity unpinned by
 * construction, validated by the certificate (feasibility, stationarity, lambda_min(P0_b + mu_b diag a_b) >= 0, for <= the sign of
 * mu and complementarity: qcqp_amd.sdr.certify_spectral_batch).
 * Outputs, any may be NULL: x [B][n] = (y - beta / (2 s)) / s; bound [B] = f0(x) recomputed from P0_b, q0_b, r0_b; mu [B];
 * lam [B][n], the eigenvalues of A_b ascending; sweeps [B]; branch [B]: 0 interior, 1 boundary, 2 hard case; status [B]: 0, 1 if
 * Jacobi stopped at max_sweeps, 2 if a result is not finite or the eigen-solver had no norm to measure against: A_b has a nonzero
 * entry but |A_b|_F^2 evaluates to 0.0 or is not finite (the point is then NOT a solution; an all-zero A_b is status 0).
 * Supported magnitudes: the squares of the entries of A_b must neither underflow nor overflow (more precisely, 2^-120 tol^2 |A_b|_F^2
 * must be a normal number and |A_b|_F^2 finite).  Inside that range multiplying (P0_b, q0_b, r0_b) by a power of two is exact: x,
 * sweeps, branch and status keep their bits, lam, mu and bound are scaled exactly (an a_pq with a_pq^2 <= 2^-120 tol^2 |A_b|_F^2 is not
 * rotated, csrc/jacobi_small.h: nothing depends on where an entry underflows).  Repeated eigenvalues slow the sweeps down to linear
 * convergence (up to 56 sweeps at n = 64 for tol = 1e-15): status 1 at max_sweeps = 30 with lam already exact to rounding.
 * QCQPMI_EUNSUPPORTED: n > 64.  QCQPMI_EINVAL: B < 1, a missing input, agg_stride other than 0 and 2 n + 1, an a_i that is not
 * positive and finite, rho^2 <= 0, a P0_b that is not symmetric.  The call works in a buffer of its own: the resident population,
 * its evaluation, its status codes and qcqpmi_last_cd_kernel stay as they were, whether the call succeeds or is refused. */
int qcqpmi_spectral_small_batch(qcqpmi_ctx *ctx, int64_t B, const double *P0s, const double *q0s, const double *r0s,
                                const double *agg, int64_t agg_stride, int relop_eq, int max_sweeps, double tol, double *x,
                                double *bound, double *mu, double *lam, int64_t *sweeps, int *branch, int *status);
/* THE SAME FOR 1 <= n <= 128 (added within ABI 6: a new symbol, nothing else changes): the arguments, outputs and status codes of
 * qcqpmi_spectral_small_batch.  n <= 64 makes exactly its launch (same kernel, same bits).  65 <= n <= 128 launches
 * spectral_wide_kernel (csrc/spectral_wide.h), still one wavefront per problem: A_b and Q_b together pass the LDS of a compute
 * unit there, so the eigen-solver is shifted one-sided (Hestenes) Jacobi on ONE array G = A_b + 2 |A_b|_F I (csrc/jacobi_wide.h;
 * a pair of columns is rotated where |g_p . g_q| > tol |g_p| |g_q|, the solver stops after the first sweep without a rotation
 * or at max_sweeps; sweeps counts that last sweep), the columns of G end as Q_b, the eigenvalues are the Rayleigh quotients
 * q_k' A_b q_k, and a lane holds two coordinates / eigen-indices.  The secular equation, the hard-case rule and the point are
 * unchanged.  The supported magnitudes and status 2 are those of qcqpmi_spectral_small_batch (the rotation threshold is relative:
 * power-of-two scaling is exact wherever the squares of the entries neither underflow nor overflow).  PAST n = 64 AN EXACT HARD CASE
 * MAY BE REPORTED AS branch == 1: the rounding of gh = Q'g, about n eps |g|, reaches the 2^-46 threshold there, so a g exactly
 * orthogonal to the lowest eigenspace keeps a component in it; mu is then within rounding of -lam_min and the value is right to
 * rounding.  QCQPMI_EUNSUPPORTED: n > 128.  QCQPMI_EINVAL and the rest as for qcqpmi_spectral_small_batch, which still refuses
 * n > 64. */
int qcqpmi_spectral_batch(qcqpmi_ctx *ctx, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *agg,
                          int64_t agg_stride, int relop_eq, int max_sweeps, double tol, double *x, double *bound, double *mu,
                          double *lam, int64_t *sweeps, int *branch, int *status);
/* IMPROVE(ADMM) FOR MANY SMALL PROBLEMS IN ONE LAUNCH (added within ABI 6: a new symbol, nothing else changes).  The batch of
 * qcqpmi_cd_small_batch_run -- B objectives P0s [B][n][n] (each symmetric), q0s [B][n], r0s [B] over this context's separable
 * constraint lists (up to four per coordinate, m >= 1 in all), 1 <= n <= 64 -- through improve_admm (qcqp.py:254-285): phase 1, x1 =
 * better(x0, z1), phase 2 with its bestx bookkeeping, better(x1, bestx); R restarts per problem, no host in the loop.  cons == NULL:
 * the context's coefficients for every problem; else [B][m][3] as qcqpmi_cd_small_batch_run_pc takes them.  rhos [B]: problem b's
 * penalty (the caller applies the rule of qcqp.py:261-278); Minvs [B][n][n]: (2 (P0_b + rho_b m I))^-1, symmetric.
 * Restart (b, r) starts from the keyed normals (seed + b seed_stride, first_index + r) of qcqpmi_pop_randn, or from X0 [B][R][n]
 * (generate = 0).  The loop, its exits and its iteration counts are those of the reference: phase 1 ends when the max violation of z
 * is < tol (iters1 = z-updates made; 0 for a start that is feasible enough, which is returned as it is), phase 2 ends after the
 * iteration in which |last_z - z| < tol or max violation > viol_lim (iters2 = iterations made, that one included), both at num_iters.
 * Separable constraints move one coordinate each: a lane holds z_i, one dual per constraint on its coordinate and the sum of their
 * operands (the state of the unit-bases path of qcqpmi_admm_run, same expressions); every projection is the reference's bracket and
 * bisection to 1e-6 on one row, bracket from p as qcqpmi_admm_set_basis derives it.  z = Minv_b (2 rho_b (S + m z) - q0_b) is summed
 * in ascending index order; f0 of a phase-2 iterate comes from the solve's right-hand side, the objective of the start, of the
 * phase-1 result and of the reported point from P0_b itself.
 * PARITY.  The iteration is the reference's up to the rounding of its sums; on constraints x_i^2 == d a last-bit difference doubles
 * with every iteration, so agreement with the reference is to 1e-9 for a few iterations per phase and a median
 * statement beyond.  A result depends on (problem b, rho_b, Minv_b, seed of b, global index) alone -- not on B, the neighbours, the
 * order of the problems, the workgroups or a split of the restarts over calls: bit for bit.  With cons, restart (b, r) is bit for bit
 * the restart of the call with B = 1, cons == NULL on a context created from problem b's own functions.
 * One persistent launch of admm_small_kernel (csrc/admm_small.hip): one wavefront per (problem, restart), lane = coordinate, Minv_b
 * (and b's coefficients) staged in LDS once per workgroup.  Outputs, any may be NULL: per restart [B R] (problem-major) iters1,
 * iters2, f0, maxviol and the points X [B][R][n]; per problem [B] the best restart as qcqpmi_cd_small_batch_run reports it.
 * qcqpmi_last_admm_kernel: "admm_small_kernel<1>" / "<4>" / "<1,pc>" / "<4,pc>" (workgroups per tile: 0).
 * Refusals, before any launch where the host can see them; the resident population, its evaluation, an installed ADMM basis and
 * qcqpmi_last_cd_kernel stay as they were, whether the call succeeds or is refused.  QCQPMI_EUNSUPPORTED: n > 64, constraints that are
 * not separable.  QCQPMI_EINVAL: B < 1, R < 1, B R >= 2^30, num_iters < 0, no constraint, a missing array, a rhos entry that is not
 * positive and finite, a cons entry that is not finite or has p == q == 0, a P0_b or Minv_b that is not symmetric (found while staging:
 * the call fails after its launch and returns no results). */
int qcqpmi_admm_small_batch_run(qcqpmi_ctx *ctx, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *cons,
                                const double *rhos, const double *Minvs, int64_t R, int generate, const double *X0, int phase1,
                                int64_t num_iters, double tol, double viol_lim, uint64_t seed, uint64_t seed_stride,
                                uint64_t first_index, double select_tol, int64_t *iters1, int64_t *iters2, double *f0, double *maxviol,
                                double *X, int64_t *best_index, double *best_f0, double *best_maxviol, double *best_x);
/* IMPROVE(ADMM) FOR PROBLEMS OF UP TO 128 VARIABLES (added within ABI 6: a new symbol, nothing else changes).  The arguments of
 * qcqpmi_admm_small_batch_run, 1 <= n <= 128.
 * n <= 64: exactly the launch of qcqpmi_admm_small_batch_run -- the same kernel, the same bits, the same name in qcqpmi_last_admm_kernel.
 * 65 <= n <= 128: the WIDE kernels admm_small_kernel<MAXC, pc, 2> -- one wavefront per (problem, restart) as before, lane l holds the
 * coordinates l and l + 64 (the second one where l + 64 < n), each with its z, its duals, its operand sum and its constraint list; the
 * keyed starts go by the coordinate index.  z = Minv_b rhs is summed over k = 0 .. n-1 ascending with rhs_k read from slot k >> 6 at
 * lane k & 63; the sums over the coordinates (f0 of an iterate, |last_z - z|^2) add the lane's two slots first and then run the tree over
 * the lanes; the objective through P0_b keeps its ascending sums across both slots.  The LDS image is the same -- Minv_b row-major
 * n x n, q0_b, the [3][m] coefficients with cons, two control words: (n^2 + n + 3 m) 8 + 8 bytes, 132 104 at n = 128 without cons, at most
 * 144 392 of the 160 KB of a CU; P0_b stays in global memory.  Workgroups of 256 or 512 threads, whichever holds more waves on a CU.
 * A 64 x 64 QPSK MIMO frame (128 real variables) is the example.
 * PARITY: that of qcqpmi_admm_small_batch_run, unchanged -- 1e-9 against the reference for a few iterations per phase; a result depends
 * on (problem b, rho_b, Minv_b, seed of b, global index) alone: bit for bit; with cons, restart (b, r) is bit for bit the restart of the
 * call with B = 1, cons == NULL on a context created from problem b's own functions.
 * qcqpmi_last_admm_kernel for n > 64: "admm_small_kernel<1,w2>" / "<4,w2>" / "<1,pc,w2>" / "<4,pc,w2>".
 * Refusals, the resident population and qcqpmi_last_cd_kernel left alone.  QCQPMI_EUNSUPPORTED: n > 128, constraints that are not
 * separable.  QCQPMI_EINVAL: everything qcqpmi_admm_small_batch_run refuses with it. */
int qcqpmi_admm_batch_run(qcqpmi_ctx *ctx, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *cons,
                          const double *rhos, const double *Minvs, int64_t R, int generate, const double *X0, int phase1,
                          int64_t num_iters, double tol, double viol_lim, uint64_t seed, uint64_t seed_stride, uint64_t first_index,
                          double select_tol, int64_t *iters1, int64_t *iters2, double *f0, double *maxviol, double *X,
                          int64_t *best_index, double *best_f0, double *best_maxviol, double *best_x);
/* IMPROVE CHAINS FOR MANY SMALL PROBLEMS IN ONE LAUNCH (added within ABI 6: a new symbol and a plain struct, nothing else changes).
 * The reference's improve takes a list of methods and runs them one after the other, each from the point the previous one left
 * (qcqp.py:420-432).  This call does that for the batch of qcqpmi_cd_small_batch_run / qcqpmi_admm_small_batch_run -- B objectives over
 * this context's separable constraint lists, 1 <= n <= 64, R restarts per problem; cons == NULL or [B][m][3] -- with 1 <= nstages <= 4
 * stages, each COORD_DESCENT (method 0: phase1, num_iters, tol, viol_tol as qcqpmi_cd_small_batch_run reads them) or ADMM (method 1:
 * phase1, num_iters, tol, viol_lim as qcqpmi_admm_small_batch_run reads them; rhos [B] and Minvs [B][n][n] as that call takes them, NULL
 * where no stage is ADMM).  Stage 0 starts from the keyed normals (seed + b seed_stride, first_index + r) or from X0 [B][R][n]
 * (generate = 0); stage s > 0 starts from the point stage s - 1 left, ALSO where that stage reported a failure for the restart (status
 * != 0, f0 = maxviol = inf): its point is handed on as it is.  Every stage keys its draws with the same (seed + b seed_stride,
 * first_index + r), as separate calls with one seed do.
 * PARITY.  The call is DEFINED as the composition of the two single calls: restart (b, r) of stage s is bit for bit what
 * qcqpmi_cd_small_batch_run[_pc] / qcqpmi_admm_small_batch_run return when they are called stage by stage with the X of one call as the X0
 * (generate = 0) of the next -- the same device functions in the same order on the same inputs -- and so inherits their parity
 * statements (the CPU oracle's improve_cd_sep term for term; 1e-9 against the reference for a few ADMM iterations per phase) and their
 * invariances: a result depends on (problem b, rho_b, Minv_b, seed of b, global index, the stages) alone, not on B, the neighbours,
 * the order of the problems, the workgroups or a split of the restarts over calls.
 * One persistent launch of chain_small_kernel (csrc/chain_small.hip): a workgroup works its ticket through all stages -- per stage it
 * replaces the LDS image (P0_b, or Minv_b), and a barrier hands the points over through global memory -- while other workgroups are
 * wherever they are: no join between the stages, no host in the loop.
 * Per-stage records, any may be NULL: st_* are arrays [nstages][B R] (stage-major, then problem-major); a CD stage fills its row of
 * st_sweeps1, st_sweeps2, st_visits2, st_accepted2, st_ran_phase2, st_status1, st_status2, an ADMM stage its row of st_iters1,
 * st_iters2, every stage its row of st_f0, st_maxviol; the rows of what a stage does not produce are zero.  f0, maxviol [B R], X
 * [B][R][n] and best_* [B] (as qcqpmi_cd_small_batch_run reports them) are those of the LAST stage.
 * qcqpmi_last_cd_kernel: "chain_small_kernel<1>" / "<4>" / "<1,pc>" / "<4,pc>".
 * Refusals, all before any launch except the symmetry check; the resident population, its evaluation, its status codes and an
 * installed ADMM basis stay as they were, whether the call succeeds or is refused.  QCQPMI_EUNSUPPORTED: n > 64, constraints that are
 * not separable.  QCQPMI_EINVAL: nstages < 1 or > 4, stages == NULL, an unknown method, an ADMM stage with rhos or Minvs NULL, and
 * everything the two single calls refuse with it (B < 1, R < 1, B R >= 2^30, num_iters < 0, a CD stage's tol <= 0, a missing array;
 * with an ADMM stage no constraint or a rhos entry that is not positive and finite; a cons entry that is not finite or has p == q ==
 * 0; a P0_b or Minv_b that is not symmetric -- found while staging: the call fails after its launch and returns no results). */
typedef struct {
    int method;        /* 0: COORD_DESCENT, 1: ADMM */
    int phase1;
    int64_t num_iters;
    double tol;        /* CD: the acceptance threshold (1e-4 in the reference); ADMM: the exit tolerance of both phases (1e-2) */
    double viol_tol;   /* CD only */
    double viol_lim;   /* ADMM only */
} qcqpmi_chain_stage;
int qcqpmi_chain_small_batch_run(qcqpmi_ctx *ctx, int64_t B, const double *P0s, const double *q0s, const double *r0s, const double *cons,
                                 const double *rhos, const double *Minvs, int64_t R, int generate, const double *X0, int nstages,
                                 const qcqpmi_chain_stage *stages, uint64_t seed, uint64_t seed_stride, uint64_t first_index,
                                 double select_tol, int64_t *st_sweeps1, int64_t *st_sweeps2, int64_t *st_visits2, int64_t *st_accepted2,
                                 uint8_t *st_ran_phase2, int *st_status1, int *st_status2, int64_t *st_iters1, int64_t *st_iters2,
                                 double *st_f0, double *st_maxviol, double *f0, double *maxviol, double *X, int64_t *best_index,
                                 double *best_f0, double *best_maxviol, double *best_x);
/* THE SETUP OF THE TWO CALLS ABOVE ON THE DEVICE (added within ABI 6: a new symbol, nothing else changes).  rhos and Minvs of
 * qcqpmi_admm_small_batch_run / qcqpmi_admm_batch_run for B problems over this context (n, m = its number of constraints, its device),
 * 1 <= n <= 128, from ONE symmetric eigendecomposition P0_b = sum_k lam_k u_k u_k' per problem inside ONE persistent launch
 * (csrc/admm_setup.h: admm_setup_kernel for n <= 64 -- cyclic Jacobi, A and Q in LDS --, admm_setup_wide_kernel for 65 <= n <= 128 --
 * shifted one-sided Jacobi on one array, eigenvalues as Rayleigh quotients; one wavefront per problem, max_sweeps and tol as
 * qcqpmi_spectral_batch passes them to the same two solvers):
 *   lambda_min[b] = min_k lam_k;
 *   rhos[b]       = rho == NULL: the rule of qcqp.py:270-277 applied to lambda_min[b], in the caller's order of operations --
 *                   lambda_min < 0 ? 50 * ((2 * (1 - lambda_min)) / m) : 50 * (1 / m) -- bit for bit (so a P0_b whose eigenvalues the
 *                   solver finds exactly, diagonal or zero, gets the bits of a host that applies the rule to LAPACK's lambda_min);
 *                   else *rho, the caller's penalty for every problem;
 *   Minvs[b]      = sum_k u_k u_k' / (2 (lam_k + rhos[b] m)) = (2 (P0_b + rhos[b] m I))^-1, every entry summed in ascending k of the
 *                   solver's order with the product u_ik u_jk formed first: EXACTLY symmetric, as the two run calls require;
 *   sweeps[b]     = Jacobi sweeps;
 *   status[b]     = 0; 1: Jacobi stopped at max_sweeps; 2: lambda_min, rho or an entry of the inverse is not finite (a given rho with
 *                   lambda_min[b] + m rho == 0 exactly: 1 / 0), or P0_b has a nonzero entry but |P0_b|_F^2 evaluates to 0.0 or is not
 *                   finite -- the squares of the entries of P0_b must neither underflow nor overflow; inside that range a
 *                   power-of-two scaling of P0_b scales lambda_min exactly --; 3: the given
 *                   rho is too small (lambda_min[b] + m rho < 0: the reference's test; Minvs[b] is then all zero).  A rho that is
 *                   too small is NOT an error of the call: the caller words the reference's message from lambda_min[b].
 * The rule jumps by a factor of about two at lambda_min = 0; for a singular positive semidefinite P0_b rounding decides the branch,
 * here as in LAPACK.  The contract: rhos[b] is the rule applied to the reported lambda_min[b], and lambda_min[b] agrees with LAPACK's
 * to rounding (a small multiple of eps |P0_b|_F).
 * A result depends on (P0_b, m, the rho argument, max_sweeps, tol) alone -- not on B, the neighbours, the order of the problems or
 * the workgroups: bit for bit.  Any output may be NULL.
 * Refusals, before any launch where the host can see them; the resident population, its evaluation, an installed ADMM basis,
 * qcqpmi_last_cd_kernel and qcqpmi_last_admm_kernel stay as they were, whether the call succeeds or is refused.
 * QCQPMI_EUNSUPPORTED: n > 128, constraints that are not separable (as the run calls).  QCQPMI_EINVAL: B < 1 (or >= 2^30), P0s
 * missing, max_sweeps < 1, tol not positive and finite, a given rho that is not positive and finite, no constraint (m < 1), a P0_b
 * that is not symmetric or holds a NaN (found while staging: the call fails after its launch and returns no results). */
int qcqpmi_admm_batch_setup(qcqpmi_ctx *ctx, int64_t B, const double *P0s, const double *rho, int max_sweeps, double tol, double *rhos,
                            double *lambda_min, double *Minvs, int64_t *sweeps, int *status);
/* Device and pinned-host buffers for a qcqpmi_cd_stream_run(K, R) to come (population, per-restart outputs, per-population
 * winners; with an objective factor set, the buffers of the factored kernel's pre-passes: slacks and Y0 = L^T x0): allocation only, so that a timed or latency-sensitive run does not start with hipMalloc / hipHostMalloc.  A
 * resident population smaller than K R points is dropped (like any reallocation of the population). */
int qcqpmi_cd_stream_reserve(qcqpmi_ctx *ctx, int64_t K, int64_t R);
/* Which lifecycle kernel qcqpmi_cd_stream_run launches: 0 (default) the faster one for the shape -- cd_life_kernel (csrc/cd_life.hip,
 * round 5) everywhere except the Boolean family at n >= 960 with more than 8192 restarts in the run, where the round-4 kernel
 * (cd_phase2_qs_kernel<lifecycle>, csrc/cd_queue.hip: Boolean family, n a multiple of 16, n <= 1024) is 12 % faster; 2: cd_life_kernel
 * wherever it applies; 1: the round-4 kernel only.  Both produce the same restarts (tests/test_gpu_life.py, tests/test_gpu_stream.py run
 * every case with both); qcqpmi_last_cd_kernel names the one that ran. */
int qcqpmi_cd_life_version(qcqpmi_ctx *ctx, int version);
/* Factored objective (round 6).  get_onevar_func (utilities.py:99-105) needs (P0 z)_i per coordinate visit; when P0 = L L^T with L
 * n x r (row-major; a least-squares objective |A x - b|^2 has L = A^T, r = rows of A; any PSD P0 of low rank has one), the lifecycle
 * kernel carries Y = L^T X per tile of restarts instead of multiplying with P0: (P0 X)[I_b, :] = L[I_b, :] Y and Y += L[I_b, :]^T (moves
 * of block b) -- 8 r / 16 matrix instructions per block of 16 coordinates instead of n / 4.  P0 itself stays uploaded (diagonal
 * blocks, the evaluation kernels, every other path); the caller vouches for L L^T = P0 (qcqp_amd.lowrank.objective_factor checks
 * it to 1e-12 of the largest entry).  Takes r <= 288 and 128 <= n <= 4096 (ABI 6), single-class separable constraints on a positive
 * diagonal (QCQPMI_EUNSUPPORTED otherwise; qcqpmi_cd_stream_run then runs as without a factor).  L == NULL or r == 0 removes it;
 * qcqpmi_cd_life_version(ctx, 3) = cd_life_kernel WITHOUT the factor (comparisons).  (A diagonal of mixed sign is not PSD: the SGN
 * kind of qcqpmi_cd_stream_run never runs with a factor.) */
int qcqpmi_cd_set_objective_factor(qcqpmi_ctx *ctx, const double *L, int64_t r);
/* Coordinate descent for constraints that couple coordinates IN THE REFERENCE'S SUMMATION ORDER (test / diagnostic mode, any
 * n): every one-variable coefficient (t2, t1, t0) of get_onevar_func (utilities.py:99-105) is formed by row-sequential sums
 * like the reference's CSR products -- t0 = f_k(z) afresh per coordinate, O((m+1) n^2) per coordinate visit -- so that
 * trajectories are comparable with the reference value for value where the MFMA path (different summation order, 1e-13
 * input noise amplified by the phase-1 bisection) is only comparable as a distribution.  Needs uploaded (not generated)
 * functions with m n^2 <= 2e9 entries.  enable = 0 restores the default dispatch. */
int qcqpmi_cd_reference_order(qcqpmi_ctx *ctx, int enable);
/* The UNIT STEP of the default dense-constraint path (products on the matrix cores + dense_chain_mw_kernel) on the resident
 * points: the coordinate visits [coord_lo, coord_hi) (0, 16 = all) of block `block` in sweep `sweep` of phase 1
 * (qcqp.py:112-141) or phase 2 (qcqp.py:160-176), started from fresh function values, with the keyed draws of that sweep.
 * phase 2: slack (R values, host) is the `viol` the reference fixes at the start of the phase (qcqp.py:157); NULL takes the
 * max violation of the resident points.  This is what the parity tests teacher-force with the states the oracle visits:
 * coordinate descent with coupled constraints is chaotic in the reference itself (one ulp of x0 moves 40 % of the dense
 * family's and every beamforming restart by > 1e-6: profiles/r04_reference_sensitivity.md, tests/test_host_cpu.py), so a
 * free-running trajectory can only be compared for bit-identical arithmetic (qcqpmi_cd_reference_order) -- the fast path is
 * compared visit by visit and block by block on the reference's own states. */
int qcqpmi_cd_dense_block_step(qcqpmi_ctx *ctx, int phase, int64_t sweep, int64_t block, int coord_lo, int coord_hi,
                               double viol_tol, double tol, uint64_t seed, uint64_t first_index, const double *slack);
/* Chain kernel of the dense-constraint path: 0 (default) dense_chain_mw_kernel -- a workgroup of four waves per restart,
 * the functions dealt to 256 threads -- whenever m + 1 <= 2048; 1: dense_chain_kernel, one wave per restart (round 1-2
 * kernel, the cross-check: the two produce the same points bit for bit). */
int qcqpmi_dense_chain_mode(qcqpmi_ctx *ctx, int mode);
/* Geometry of dense_chain_mw_kernel for m constraints (host-only, no device call): out4 = {slots per thread, threads that
 * hold constraints Tc, index of the serial thread (holds the objective), threads per restart}.  Constraint k = 1..m is
 * slot (k - 1) / Tc of thread (k - 1) % Tc.  More than 8 slots: the one-wave kernel is used instead. */
int qcqpmi_dense_chain_geometry(int64_t m, int *out4);
int qcqpmi_sync(qcqpmi_ctx *ctx);
/* debug: enable in-kernel cycle counters of the phase-2 kernel / read their sums over tiles
 * (slots: 0 mfma, 1 feasible sets, 2 barrier, 3 sequential part, 4 barrier, 5 #blocks) */
int qcqpmi_debug_profile(qcqpmi_ctx *ctx, int enable, int64_t *sums8);
/* debug: stage cycle counters (s_memtime ticks of member 0 of tile 0) of the last fused ADMM run made while
 * qcqpmi_debug_profile(ctx, 1, NULL) was on: 0 z-update, 1 partial product, 2 exchange 1, 3 sums, 4 secular solves,
 * 5 exchange 2, 6 gather, 7 bookkeeping, 9 iterations */
int qcqpmi_debug_admm_profile(qcqpmi_ctx *ctx, int64_t *out16);
/* debug: stage tick sums (s_memtime) of the dense chain kernel's wave of restart 0 over the runs made while
 * qcqpmi_debug_profile(ctx, 1, NULL) was on (library built with -DDN_PROFILE=1, else zeros): [0..15] phase 1, [16..31]
 * phase 2 of the serial thread (one-wave kernel: the wave), [32..63] the same for thread 0 of the multi-wave kernel.
 * Slots: 0 set-up, 1 one-variable coefficients, 2 bounds + reductions, 3 gaps, 4 segment sweep, 5 minimiser / draw,
 * 6 commit, 7 write-back, 8 coordinates visited, 9 feasible-set evaluations.  Reading resets the sums. */
int qcqpmi_debug_dense_profile(qcqpmi_ctx *ctx, int64_t *out64);
/* debug: per-wave event trace (cycle stamps) of tile 0 of the last profiled phase-2 run; count <= 2048 words */
int qcqpmi_debug_trace(qcqpmi_ctx *ctx, int64_t *out, int count);

/* ---- multi-GPU: one process per GPU, restarts sharded by global index, ONE collective at the
 * end to pick the global best (RCCL over xGMI; librccl is loaded lazily). --------------- */
int qcqpmi_comm_unique_id(uint8_t id_out[128]);
int qcqpmi_comm_init(qcqpmi_ctx *ctx, int rank, int world, const uint8_t id[128]);
/* all ranks call; local best (from qcqpmi_select_best semantics) -> global best on every rank.
 * index_offset = global index of this rank's candidate 0. */
int qcqpmi_comm_select_best(qcqpmi_ctx *ctx, double tol, int64_t index_offset,
                            int64_t *best_global_index, double *best_f0, double *best_maxviol,
                            double *best_x);
int qcqpmi_comm_barrier(qcqpmi_ctx *ctx);
/* in-place all-reduce of host doubles (RCCL all-reduce of a device copy); op 0 = max, 1 = sum (bench.py: max-over-ranks
 * step time, sum-over-ranks work counters; the exchange of a streamed run: the table of the local winners' keys of all
 * populations, then the table of the winners' points -- qcqp_amd.dist.global_best_of_populations) */
int qcqpmi_comm_allreduce(qcqpmi_ctx *ctx, double *values, int64_t count, int op);
/* all-gather of host bytes (ABI 5): every rank contributes nbytes bytes, recv receives world x nbytes bytes in rank order -- one
 * ncclAllGather.  The exchange of a streamed run uses it for the local winners' KEYS: 32 bytes per population and rank -- the
 * QCQPForm.better bucket int(maxviol / tol) (utilities.py:139-140), the objective, the max violation, the GLOBAL restart index
 * (int64: exact; the ticket cap K R < 2^30 of qcqpmi_cd_stream_run bounds it per rank, not per job) -- then ONE sum-all-reduce of
 * the K winners' points with only the owner's rows filled (qcqp_amd.dist.global_best_of_populations). */
int qcqpmi_comm_allgather(qcqpmi_ctx *ctx, const void *send, int64_t nbytes, void *recv);

#ifdef __cplusplus
}
#endif
#endif
