"""QCQPBatch: many SMALL problems that share their constraints -- or the structure of their constraints --, solved in one launch.

A frame of MIMO detection problems is thousands of independent Boolean least squares instances of 8 .. 128 variables: every
instance has its own objective and all of them the constraints x_i^2 == 1.  ``QCQP`` holds one problem per context; this class
holds B of them on ONE context and runs suggest(RANDOM) + improve(COORD_DESCENT) for all B x R restarts through one persistent
kernel (``Engine.cd_small_batch_run``, qcqpmi_cd_small_batch_run; for 64 < n <= 128 ``Engine.cd_batch_run``, qcqpmi_cd_batch_run: the
wide kernels, two coordinates per lane).  improve(ADMM) runs the reference's consensus ADMM for all B x R restarts in one launch too
(n <= 64: ``Engine.admm_small_batch_run``, qcqpmi_admm_small_batch_run; 64 < n <= 128, asked for with wide=True:
``Engine.admm_batch_run``, qcqpmi_admm_batch_run, wide kernels again), with rho per problem by the reference's rule and
(2 (P0_b + rho_b m I))^-1 from one batched host inverse -- or, with setup='device', both from one eigendecomposition per problem in
one more launch (``Engine.admm_batch_setup``, qcqpmi_admm_batch_setup).  suggest(SDR) -- for constraints x_i^2 == d_i -- solves the
semidefinite relaxation of all B problems and draws their samples in one launch as well (n <= 64: ``Engine.sdr_small_batch``,
qcqpmi_sdr_small_batch; 64 < n <= 128, asked for with wide=True: ``Engine.sdr_batch``, qcqpmi_sdr_batch, the wide kernel with C_b
packed in LDS) and publishes the certified bounds in ``sdr_bound``; improve() then starts from the samples.  suggest(SPECTRAL) --
for constraints of ONE relop that sum to a sphere or a ball (Boolean, x_i^2 == d_i, MAXCUT, boxes), n <= 64 -- solves the reference's
spectral relaxation of all B problems exactly in one launch (``Engine.spectral_small_batch``, qcqpmi_spectral_small_batch: one
eigendecomposition and one secular equation per problem; 64 < n <= 128, asked for with wide=True: ``Engine.spectral_batch``,
qcqpmi_spectral_batch, the wide kernel with ONE array of the eigen-solver in LDS) and publishes ``spectral_sol`` and ``spectral_bound``.  Problem b's results are those of
``QCQP(Problem(funcs_b))`` with suggest(RANDOM, num_samples=R, seed=seed + b seed_stride, first_index=...) followed by
improve(COORD_DESCENT, ..., seed=seed + b seed_stride, first_index=...).  Problems whose constraints differ in their COEFFICIENTS
only (boxes with bounds per instance, x_i^2 == d_{b,i}: problems.per_problem_constraints_batch) run through the same launches with
per-problem coefficients.  suggest(SDR) takes n <= 64 by default and n <= 128 with wide=True (the LDS image of the relaxation fits a
CU up to n = 128 once C_b is stored as its lower triangle).

    from qcqp_amd.batch import QCQPBatch
    from qcqp_amd import problems, settings as s
    batch = QCQPBatch(problems.boolean_least_squares_batch(B=4096, n=32, m=48, seed=1))
    batch.suggest(s.RANDOM, num_samples=64, seed=7)
    f, v = batch.improve(s.COORD_DESCENT)          # (B,), (B,): the best restart of every problem
    batch.x                                        # (B, n)
    batch.suggest(s.SDR, num_samples=64, seed=7)   # the SDR detector: batch.sdr_bound (B,), samples of N(mu_b, Sigma_b)
    f, v = batch.improve(s.COORD_DESCENT)
    batch.suggest(s.RANDOM, num_samples=64, seed=7)
    f, v = batch.improve(s.ADMM, num_iters=100)    # batch.last_stats['rho'] (B,), ['iters1'], ['iters2'] (B, R)
    f, v = batch.improve([s.ADMM, s.COORD_DESCENT], num_iters=100)     # a chain: ADMM, then coordinate descent from its points,
                                                   # n <= 64 and up to 4 stages in ONE launch (Engine.chain_small_batch_run)
"""
import numpy as np
import scipy.sparse as sp

from . import sdr as _sdr
from . import settings as s
from .engine import Engine
from .form import QCQPForm


def _dense(P):
    return np.asarray(P.toarray() if sp.issparse(P) else P, dtype=np.float64)


def _same_constraints(fa, fb):
    if len(fa) != len(fb):
        return False
    for (Pa, qa, ra, oa), (Pb, qb, rb, ob) in zip(fa[1:], fb[1:]):
        if oa != ob or float(ra) != float(rb):
            return False
        if not np.array_equal(np.asarray(qa, dtype=np.float64).ravel(), np.asarray(qb, dtype=np.float64).ravel()):
            return False
        if Pa is not Pb and not np.array_equal(_dense(Pa), _dense(Pb)):
            return False
    return True


def _entry(P, q, r, relop):
    """(coordinate, relop, p, q, r) of a constraint that touches ONE coordinate -- p = P[i,i], q = q[i]: what qcqpmi_finalize keeps per
    list entry -- or None for any other constraint (coupled, or constant).  The stored entries of a sparse P count as touched, zero or
    not, as the context counts them."""
    q = np.asarray(q, dtype=np.float64).ravel()
    if sp.issparse(P):
        Pc = P.tocoo()
        rows, cols, vals = Pc.row, Pc.col, Pc.data
    else:
        Pd = np.asarray(P, dtype=np.float64)
        rows, cols = np.nonzero(Pd)
        vals = Pd[rows, cols]
    touched = set(int(i) for i in rows) | set(int(j) for j in cols) | set(int(j) for j in np.nonzero(q)[0])
    if len(touched) != 1:
        return None
    i = touched.pop()
    return i, relop, float(np.sum(vals)), float(q[i]), float(r)


def _structure(funcs):
    """The entries of every constraint, or None if one of them is not separable."""
    out = [_entry(*f) for f in funcs[1:]]
    return None if any(e is None for e in out) else out


MAX_N = 128          # qcqpmi_cd_batch_run, qcqpmi_admm_batch_run, qcqpmi_sdr_batch: two coordinates per lane
MAX_N_SMALL = 64     # qcqpmi_cd_small_batch_run, qcqpmi_sdr_small_batch, qcqpmi_admm_small_batch_run: one coordinate per lane


def admm_rhos(P0s, m, rho=None):
    """The rho rule of improve_admm (qcqp.py:261-278) for every problem, from ONE batched eigvalsh of P0s (B, n, n): rho == None gives
    50 * 2 (1 - lambda_min) / m where lambda_min < 0 and 50 / m elsewhere; a given rho is checked against lambda_min + m rho >= 0 and
    the reference's exception names the first problem that fails.  Returns rhos (B,)."""
    P0s = np.asarray(P0s, dtype=np.float64)
    lmin = np.linalg.eigvalsh(P0s)[:, 0]
    if rho is not None:
        rho = float(rho)
        bad = np.nonzero(lmin + m * rho < 0)[0]
        if bad.size:
            raise Exception(rho_too_small_message(rho, bad[0], lmin[bad[0]], m))
        return np.full(P0s.shape[0], rho)
    return 50. * np.where(lmin < 0, 2. * (1. - lmin) / m, 1. / m)


def rho_too_small_message(rho, b, lmin_b, m):
    """The reference's exception text for a given rho that is too small, naming problem b (lmin_b: its lambda_min)."""
    return ("rho parameter is too small, need at least %.3f. (problem %d: minimum possible value %.3f)" % (rho, int(b), -lmin_b / m))


def admm_minvs(P0s, rhos, m):
    """(2 (P0_b + rho_b m I))^-1 for every problem: one batched inverse, symmetrised (the kernel reads columns as rows)."""
    P0s = np.asarray(P0s, dtype=np.float64)
    n = P0s.shape[1]
    Mi = np.linalg.inv(2. * (P0s + (np.asarray(rhos) * m)[:, None, None] * np.eye(n)))
    return (Mi + Mi.transpose(0, 2, 1)) / 2.


CHAIN_STAGE_KEYS = ('num_iters', 'tol', 'viol_tol', 'viol_lim', 'phase1')
FUSED_MAX_STAGES = 4     # qcqpmi_chain_small_batch_run: stages per launch (n <= MAX_N_SMALL)


def chain_stages(method, num_iters=1000, viol_tol=1e-2, tol=None, phase1=True, viol_lim=1e4):
    """The stage descriptors of QCQPBatch.improve(method, ...): ``method`` is a method or a list whose entries are a method or
    (method, kwargs) with that stage's own num_iters / tol / viol_tol / viol_lim / phase1; the keyword arguments are the default of
    every stage (the reference hands one **kwargs to every method of its list, qcqp.py:420-432).  tol == None stands for each method's
    own default: 1e-4 for COORD_DESCENT, 1e-2 for ADMM.  Returns a list of dictionaries with the keys method, phase1, num_iters, tol,
    viol_tol, viol_lim.  A pure function: no device, no library."""
    entries = list(method) if isinstance(method, list) else [method]
    if not entries:
        raise Exception("QCQPBatch.improve: the list of methods is empty")
    defaults = dict(num_iters=num_iters, tol=tol, viol_tol=viol_tol, viol_lim=viol_lim, phase1=phase1)
    out = []
    for k, e in enumerate(entries):
        meth, kw = (e[0], dict(e[1])) if isinstance(e, tuple) and len(e) == 2 and isinstance(e[1], dict) else (e, {})
        if meth not in (s.COORD_DESCENT, s.ADMM):
            raise Exception("QCQPBatch.improve is defined for the COORD_DESCENT and ADMM methods")
        unknown = sorted(set(kw) - set(CHAIN_STAGE_KEYS))
        if unknown:
            raise Exception("QCQPBatch.improve: stage %d has the argument %r; a stage takes %s" % (k, unknown[0], ', '.join(CHAIN_STAGE_KEYS)))
        g = dict(defaults, **kw)
        if g['tol'] is None:
            g['tol'] = 1e-4 if meth == s.COORD_DESCENT else 1e-2
        out.append(dict(method=meth, phase1=bool(g['phase1']), num_iters=int(g['num_iters']), tol=float(g['tol']),
                        viol_tol=float(g['viol_tol']), viol_lim=float(g['viol_lim'])))
    return out


class QCQPBatch(object):
    """``funcs_list`` = [funcs_0, ..., funcs_{B-1}], every funcs_b = [(P, q, r, relop), ...] in minimise form with the objective
    first (what qcqp_amd.problems returns).  All problems must have the same n (<= 128; suggest(SDR) and improve(ADMM) past 64: with wide=True) and constraints of the same STRUCTURE: the
    same number of them, and constraint k with the same relop on the same coordinate in every problem.  Their coefficients may
    differ from problem to problem (separable constraints only): ``cons`` (B, m, 3) then holds (p, q, r) of every constraint and the
    launches are qcqpmi_cd_small_batch_run_pc / qcqpmi_sdr_small_batch_pc; with equal coefficients ``cons`` is None and the calls are
    those for shared constraints."""

    def __init__(self, funcs_list, device=0):
        funcs_list = [list(f) for f in funcs_list]
        if not funcs_list:
            raise Exception("QCQPBatch: empty list of problems")
        n = int(np.asarray(funcs_list[0][0][1]).size)
        for b, funcs in enumerate(funcs_list):
            nb = int(np.asarray(funcs[0][1]).size)
            if nb != n:
                raise Exception("QCQPBatch: problem %d has n = %d, problem 0 has n = %d" % (b, nb, n))
        if n > MAX_N:
            raise Exception("QCQPBatch: n = %d, the batch kernels take n <= %d (use QCQP, one context per problem)" % (n, MAX_N))
        differing = [b for b in range(1, len(funcs_list)) if not _same_constraints(funcs_list[0], funcs_list[b])]
        self.cons = None
        if differing:
            st0 = _structure(funcs_list[0])
            cons = np.empty((len(funcs_list), len(funcs_list[0]) - 1, 3))
            for b, funcs in enumerate(funcs_list):
                st = st0 if b == 0 else _structure(funcs)
                if st0 is None or st is None or len(st) != len(st0) or any(e[:2] != e0[:2] for e, e0 in zip(st, st0)):
                    raise Exception("QCQPBatch: the constraints of problem %d differ from those of problem 0 in their structure (number, "
                                    "touched coordinate or relop; only the coefficients of separable constraints may differ)"
                                    % (b if st0 is not None else differing[0]))
                cons[b] = [e[2:] for e in st]
            self.cons = cons
            self._coords = np.array([e[0] for e in st0])
        self.B, self.n = len(funcs_list), n
        self.P0s = np.empty((self.B, n, n))
        self.q0s = np.empty((self.B, n))
        self.r0s = np.empty(self.B)
        for b, funcs in enumerate(funcs_list):
            P = _dense(funcs[0][0])
            self.P0s[b] = (P + P.T) / 2.          # like get_qcqp_form (utilities.py:333)
            self.q0s[b] = np.asarray(funcs[0][1], dtype=np.float64).ravel()
            self.r0s[b] = float(funcs[0][2])
        self.form = QCQPForm.from_arrays(funcs_list[0])
        self.engine = Engine(self.form, device=device)
        self._suggested = None
        self._starts = None          # (B, R, n): the samples of suggest(SDR), the point of suggest(SPECTRAL) (R = 1); None: improve() draws the keyed normals itself
        self.sdr_bound = None
        self.sdr_info = None
        self.spectral_sol = None
        self.spectral_bound = None
        self.spectral_info = None
        self.x = None
        self.population_f = None
        self.population_v = None
        self.best_index = None
        self.last_stats = None

    def suggest(self, method=s.RANDOM, num_samples=1, seed=0, first_index=0, seed_stride=1, max_sweeps=5000, tol=1e-11, wide=False,
                certify=False, jacobi_sweeps=30, jacobi_tol=1e-15):
        """RANDOM: R = num_samples random starts per problem: problem b draws the keyed normals (seed + b seed_stride, first_index + r).
        The points are drawn inside the launch of improve(); nothing runs here.
        SDR (constraints x_i^2 == d_i): one launch solves the relaxation of every problem (mixing method, max_sweeps / tol) and
        draws R samples of N(mu_b, Sigma_b) from the keyed normals (seed + b seed_stride, first_index + r); every solve is certified
        (sdr.certify_batch, which logs the warning for problems that are not certified).  Sets .sdr_bound (B,) -- the rigorous lower bound, NaN where the problem is not certified -- and
        .sdr_info (primal, sweeps, lambda_min, converged); the samples are the starts of improve().
        wide=True admits 65 <= n <= 128 to SDR (``Engine.sdr_batch``: the wide kernel, C_b packed, two coordinates per lane in the
        samples) and to SPECTRAL (``Engine.spectral_batch``: the wide kernel, one-sided Jacobi on one array in LDS, two eigen-indices
        per lane; jacobi_tol is then the relative threshold of a rotation); n <= 64 runs as without it.  The default refuses n > 64
        as before.  RANDOM ignores it.
        SPECTRAL (n <= 64, with wide=True n <= 128; constraints that all carry ONE relop and sum to sum_i (a_i x_i^2 + beta_i x_i) + gamma with every
        a_i > 0 and rho^2 = sum beta_i^2 / (4 a_i) - gamma > 0: Boolean, x_i^2 == d_i, MAXCUT, boxes (x - lo)(x - hi) <= 0 or == 0,
        shared or per problem): one launch (``Engine.spectral_small_batch``) solves the reference's spectral relaxation of every
        problem EXACTLY -- with one aggregated constraint it is a trust-region problem: one Jacobi eigendecomposition
        (jacobi_sweeps, jacobi_tol) and one secular equation per problem.  num_samples must be 1 (the reference's SPECTRAL yields
        one point).  Sets .spectral_sol (B, n) and .spectral_bound (B,) -- the relaxation's value, a lower bound of every point
        feasible for the problem; both NaN where the launch reports a status != 0 -- and .spectral_info (mu, lam_min, sweeps,
        branch, status; with certify=True also the host certificate of sdr.certify_spectral_batch under 'certificate').  The point is
        the single start of improve()."""
        if method not in (s.RANDOM, s.SDR, s.SPECTRAL):
            raise Exception("QCQPBatch.suggest is defined for the RANDOM, SDR and SPECTRAL methods")
        if int(num_samples) < 1:
            raise Exception("QCQPBatch.suggest: num_samples must be positive")
        if method == s.SPECTRAL:
            return self._suggest_spectral(int(num_samples), seed, first_index, seed_stride, certify, jacobi_sweeps, jacobi_tol, wide)
        if method == s.SDR:
            if self.n > MAX_N_SMALL and not wide:      # before any launch
                raise Exception("QCQPBatch.suggest(SDR) is defined for n <= %d (n = %d) unless wide=True is given (n <= %d: the wide "
                                "kernel, C_b packed in LDS); or use suggest(RANDOM), or QCQP per problem" % (MAX_N_SMALL, self.n, MAX_N))
            d = _sdr.unit_diagonal_family(self.form)
            if d is None:
                raise Exception("QCQPBatch.suggest(SDR) is defined for constraints x_i^2 == d_i (one per coordinate)")
            ds = None
            if self.cons is not None:      # the family test problem by problem: p x_i^2 + r == 0 with d_b = -r / p > 0, no linear term
                p, q, r = self.cons[:, :, 0], self.cons[:, :, 1], self.cons[:, :, 2]
                ds = np.empty((self.B, self.n))
                with np.errstate(divide='ignore', invalid='ignore'):
                    ds[:, self._coords] = -r / p
                bad = np.any(q != 0.0, axis=1) | ~np.all((ds > 0.0) & np.isfinite(ds), axis=1)
                if bad.any():
                    raise Exception("QCQPBatch.suggest(SDR) is defined for constraints x_i^2 == d_i (one per coordinate): problem %d is "
                                    "not of the family" % int(np.nonzero(bad)[0][0]))
                d = ds
            run = self.engine.sdr_small_batch if self.n <= MAX_N_SMALL else self.engine.sdr_batch
            out = run(self.P0s, self.q0s, self.r0s, int(num_samples), max_sweeps=max_sweeps, tol=tol, seed=seed, seed_stride=seed_stride,
                      first_index=first_index, want_V=False, ds=ds)
            cert = _sdr.certify_batch(_sdr.lifted_cost_batch(self.P0s, self.q0s, self.r0s, d), out['y'], out['sweeps'], max_sweeps)
            self.sdr_bound = np.where(cert['converged'], cert['bound'], np.nan)
            self.sdr_info = dict(primal=out['primal'], sweeps=out['sweeps'], lambda_min=cert['lambda_min'], converged=cert['converged'])
            self._starts = out['X']
        else:
            self._starts = None
        self._suggested = (int(num_samples), int(seed), int(first_index), int(seed_stride))

    def _spectral_aggregate(self):
        """(agg, relop) of suggest(SPECTRAL): agg = [a (n) | beta (n) | gamma], the sums of (p, q, r) over the constraints, of shape
        (2 n + 1,) for shared constraints and (B, 2 n + 1) for per-problem coefficients; raises outside the family."""
        name, n = "QCQPBatch.suggest(SPECTRAL)", self.n
        entries = [_entry(f.P, f.qarray, f.r, f.relop) for f in self.form.fs]
        if not entries:
            raise Exception("%s: the problems have no constraint (nothing to aggregate)" % name)
        for k, e in enumerate(entries):
            if e is None:
                raise Exception("%s is defined for separable constraints p x_i^2 + q x_i + r (relop) 0: constraint %d couples "
                                "coordinates or touches none" % (name, k))
            if e[1] != entries[0][1]:
                raise Exception("%s is defined for constraints that all carry the same relop (all == or all <=): constraint %d is %s, "
                                "constraint 0 is %s" % (name, k, e[1], entries[0][1]))
        coords = np.array([e[0] for e in entries])
        pqr = np.array([e[2:] for e in entries])[None] if self.cons is None else self.cons      # (1 or B, m, 3)
        agg = np.zeros((pqr.shape[0], 2 * n + 1))
        np.add.at(agg[:, :n], (slice(None), coords), pqr[:, :, 0])
        np.add.at(agg[:, n:2 * n], (slice(None), coords), pqr[:, :, 1])
        agg[:, 2 * n] = pqr[:, :, 2].sum(axis=1)
        a, beta, gamma = agg[:, :n], agg[:, n:2 * n], agg[:, 2 * n]
        where = (lambda b: " of problem %d" % b) if self.cons is not None else (lambda b: "")
        bad = np.argwhere(~((a > 0.0) & np.isfinite(a)))
        if bad.size:
            b, i = int(bad[0][0]), int(bad[0][1])
            raise Exception("%s is defined for a_i > 0 on every coordinate: coordinate %d%s has a = %g (the sum of p over its constraints; "
                            "a coordinate with linear constraints only, or with none)" % (name, i, where(b), a[b, i]))
        rho2 = np.sum(beta * beta / (4. * a), axis=1) - gamma
        bad = np.nonzero(~((rho2 > 0.0) & np.isfinite(rho2)))[0]
        if bad.size:
            b = int(bad[0])
            raise Exception("%s is defined for rho^2 = sum_i beta_i^2 / (4 a_i) - gamma > 0: rho^2 = %g%s (the aggregated constraint "
                            "admits at most one point)" % (name, rho2[b], where(b)))
        return (agg[0] if self.cons is None else agg), entries[0][1]

    def _suggest_spectral(self, num_samples, seed, first_index, seed_stride, certify, jacobi_sweeps, jacobi_tol, wide=False):
        if num_samples != 1:
            raise Exception("QCQPBatch.suggest(SPECTRAL) yields one point per problem: num_samples must be 1 (num_samples = %d)" % num_samples)
        if self.n > MAX_N_SMALL and not wide:      # before any launch
            raise Exception("QCQPBatch.suggest(SPECTRAL) is defined for n <= %d (n = %d): A_b and Q_b of the eigen-solver fit a wavefront's "
                            "LDS up to there, unless wide=True is given (n <= %d: the wide kernel, one array in LDS); or use "
                            "suggest(RANDOM), or QCQP per problem" % (MAX_N_SMALL, self.n, MAX_N))
        agg, relop = self._spectral_aggregate()
        run = self.engine.spectral_small_batch if self.n <= MAX_N_SMALL else self.engine.spectral_batch
        out = run(self.P0s, self.q0s, self.r0s, agg, relop, max_sweeps=jacobi_sweeps, tol=jacobi_tol)
        ok = out['status'] == 0
        self.spectral_sol = np.where(ok[:, None], out['x'], np.nan)
        self.spectral_bound = np.where(ok, out['bound'], np.nan)
        self.spectral_info = dict(mu=out['mu'], lam_min=out['lam'][:, 0], sweeps=out['sweeps'], branch=out['branch'], status=out['status'])
        if certify:
            self.spectral_info['certificate'] = _sdr.certify_spectral_batch(self.P0s, self.q0s, agg, relop, out['x'], out['mu'])
        self._starts = np.ascontiguousarray(out['x'][:, None, :])
        self._suggested = (1, int(seed), int(first_index), int(seed_stride))

    def improve(self, method=s.COORD_DESCENT, num_iters=1000, viol_tol=1e-2, tol=None, phase1=True, seed=None, viol_lim=1e4, rho=None,
                wide=False, setup='host', fused=None):
        """improve(COORD_DESCENT) or improve(ADMM) of every suggested start of every problem; returns (f (B,), v (B,)) of the best
        restart per problem (QCQPForm.better, ties -> lowest index) and sets .x (B, n), .population_f / .population_v (B, R),
        .best_index, .last_stats.  seed: the seed of suggest() (a problem's normals and its draws come from ONE keyed stream).
        COORD_DESCENT: num_iters, viol_tol, tol (1e-4), phase1.
        ADMM (n <= 64; n <= 128 with wide=True): num_iters, tol (1e-2), viol_lim, rho, phase1 -- the arguments of the reference's
        improve_admm.  rho == None: the reference's rule (qcqp.py:270-277) problem by problem; a given rho that is too small for some
        problem raises the reference's message.  .last_stats holds rho (B,), iters1, iters2 (B, R) and the kernel's name.
        wide=True admits 65 <= n <= 128 to ADMM (``Engine.admm_batch_run``: the wide kernels, two coordinates per lane); n <= 64 runs
        as without it.  The default refuses n > 64 as before.  COORD_DESCENT ignores it.
        setup (ADMM): where rho_b and (2 (P0_b + rho_b m I))^-1 come from.  'host' (the default): one batched eigvalsh and one batched
        inverse (admm_rhos, admm_minvs).  'device': ``Engine.admm_batch_setup`` -- one launch, one Jacobi eigendecomposition per
        problem -- and then the same ADMM launch with its rho and its inverse; the rule is applied to the device's lambda_min, which
        agrees with eigvalsh to rounding (for a singular PSD P0_b rounding decides the rule's branch, here as on the host); a problem
        whose decomposition did not converge or is not finite raises.  .last_stats gains setup, lambda_min and setup_sweeps (None
        on the host path).  setup='device' does not admit n > 64 by itself (wide=True does).  COORD_DESCENT ignores it.
        A LIST of methods (the reference's improve, qcqp.py:420-432) runs them one after the other, each from the points the previous
        one left -- also those of restarts it reported as failed --, every stage with the same keyed stream.  An entry is a method
        or (method, kwargs) with that stage's own num_iters / tol / viol_tol / viol_lim / phase1; the keyword arguments of the call
        are every stage's default (chain_stages): improve([COORD_DESCENT, (ADMM, dict(phase1=False))]) is the reference's
        improve(COORD_DESCENT); improve(ADMM, phase1=False).  A list of one entry is the scalar call.  rho and setup serve every ADMM
        stage (computed once); wide is asked for as before when a stage is ADMM and n > 64.
        fused (lists only): None -- ONE launch (``Engine.chain_small_batch_run``, qcqpmi_chain_small_batch_run) where the chain kernel
        takes the problem (n <= 64, at most 4 stages), else the COMPOSED path: the engine calls of the scalar methods stage by stage,
        X of one as X0 of the next (any n <= 128, any number of stages); True -- raise, before any launch, where the chain kernel does
        not take the problem; False -- always composed.  Both paths give the same bits.  .x, .best_index, .population_f / _v and the
        returned (f, v) are the LAST stage's; .last_stats holds the last stage's arrays, method (the list), stages (one dictionary
        per stage: its method, its records, f0, maxviol), fused (bool) and kernel; with an ADMM stage also rho, setup, lambda_min,
        setup_sweeps; where the last stage is COORD_DESCENT also failed_restarts.  Two separate improve() calls still each start
        from suggest()'s points."""
        if isinstance(method, list):
            stages = chain_stages(method, num_iters=num_iters, viol_tol=viol_tol, tol=tol, phase1=phase1, viol_lim=viol_lim)
            if len(stages) > 1:
                return self._improve_chain(stages, seed, rho, wide, setup, fused)
            g = stages[0]      # exactly the scalar call
            method, num_iters, viol_tol, tol, phase1, viol_lim = g['method'], g['num_iters'], g['viol_tol'], g['tol'], g['phase1'], g['viol_lim']
        if method not in (s.COORD_DESCENT, s.ADMM):
            raise Exception("QCQPBatch.improve is defined for the COORD_DESCENT and ADMM methods")
        if method == s.ADMM and setup not in ('host', 'device'):      # before any launch
            raise Exception("QCQPBatch.improve(ADMM): setup must be 'host' or 'device' (setup = %r)" % (setup,))
        if method == s.ADMM and self.n > MAX_N_SMALL and not wide:      # before any launch
            raise Exception("QCQPBatch.improve(ADMM) is defined for n <= %d (n = %d) unless wide=True is given (n <= %d: the wide kernels, "
                            "two coordinates per lane); or use improve(COORD_DESCENT), or QCQP per problem" % (MAX_N_SMALL, self.n, MAX_N))
        if self._suggested is None:
            raise Exception("QCQPBatch.improve: call suggest(RANDOM or SDR, num_samples=R, seed=...) first")
        R, sd, first_index, stride = self._suggested
        if seed is not None and int(seed) != sd:
            raise Exception("QCQPBatch.improve: seed %d differs from the seed of suggest (%d); the batch runs one keyed stream per problem"
                            % (int(seed), sd))
        if method == s.ADMM:
            return self._improve_admm(R, sd, first_index, stride, num_iters, 1e-2 if tol is None else tol, viol_lim, rho, phase1, setup)
        tol = 1e-4 if tol is None else tol
        run = self.engine.cd_small_batch_run if self.n <= MAX_N_SMALL else self.engine.cd_batch_run
        out = run(self.P0s, self.q0s, self.r0s, R, X0=self._starts, phase1=phase1, num_iters=num_iters, viol_tol=viol_tol,
                  tol=tol, seed=sd, seed_stride=stride, first_index=first_index, want_x=False, cons=self.cons)
        failed = int(np.count_nonzero((out['status1'] != 0) | (out['status2'] != 0)))
        return self._publish(out, method, R, failed_restarts=failed, kernel=self.engine.last_cd_kernel())

    def _publish(self, out, method, R, **stats):
        """Publishes an improve launch (.x, .best_index, .population_f / _v, .last_stats); returns (f, v) of every problem's best restart."""
        self.x = out['best_x']
        self.best_index = out['best_index']
        self.population_f, self.population_v = out['f0'], out['maxviol']
        self.last_stats = dict(out, method=method, num_problems=self.B, num_restarts=R, **stats)
        return out['best_f0'], out['best_maxviol']

    def _admm_setup_device(self, m, rho):
        """(rhos, Minvs, lambda_min, sweeps) from Engine.admm_batch_setup; raises what admm_rhos raises for a rho that is too small,
        and for a decomposition that cannot be used."""
        out = self.engine.admm_batch_setup(self.P0s, rho=rho)
        short = np.nonzero(out['status'] == 3)[0]
        if short.size:
            raise Exception(rho_too_small_message(float(rho), short[0], out['lambda_min'][short[0]], m))
        failed = np.nonzero(out['status'] != 0)[0]
        if failed.size:
            b = int(failed[0])
            raise Exception("QCQPBatch.improve(ADMM, setup='device'): the eigendecomposition of P0 of problem %d %s (status %d, %d "
                            "sweeps); its inverse is not used -- setup='host' takes LAPACK's"
                            % (b, "did not converge" if out['status'][b] == 1 else "is not finite", int(out['status'][b]), int(out['sweeps'][b])))
        return out['rho'], out['Minv'], out['lambda_min'], out['sweeps']

    def _improve_admm(self, R, sd, first_index, stride, num_iters, tol, viol_lim, rho, phase1, setup='host'):
        m = self.form.m
        if setup == 'device':
            rhos, minvs, lmin, sweeps = self._admm_setup_device(m, rho)
        else:
            rhos = admm_rhos(self.P0s, m, rho)
            minvs, lmin, sweeps = admm_minvs(self.P0s, rhos, m), None, None
        run = self.engine.admm_small_batch_run if self.n <= MAX_N_SMALL else self.engine.admm_batch_run
        out = run(self.P0s, self.q0s, self.r0s, R, rhos, minvs, X0=self._starts, phase1=phase1, num_iters=num_iters,
                  tol=tol, viol_lim=viol_lim, seed=sd, seed_stride=stride, first_index=first_index, want_x=False, cons=self.cons)
        return self._publish(out, s.ADMM, R, rho=rhos, kernel=self.engine.last_admm_kernel()[0], setup=setup, lambda_min=lmin,
                             setup_sweeps=sweeps)

    def _improve_chain(self, stages, seed, rho, wide, setup, fused):
        """improve([method, ...]) with two or more stages (chain_stages): one launch of the chain kernel, or the composed path."""
        any_admm = any(g['method'] == s.ADMM for g in stages)
        can_fuse = self.n <= MAX_N_SMALL and len(stages) <= FUSED_MAX_STAGES
        # every refusal before any launch
        if any_admm and setup not in ('host', 'device'):
            raise Exception("QCQPBatch.improve(ADMM): setup must be 'host' or 'device' (setup = %r)" % (setup,))
        if any_admm and self.n > MAX_N_SMALL and not wide:
            raise Exception("QCQPBatch.improve(ADMM) is defined for n <= %d (n = %d) unless wide=True is given (n <= %d: the wide kernels, "
                            "two coordinates per lane); or use improve(COORD_DESCENT), or QCQP per problem" % (MAX_N_SMALL, self.n, MAX_N))
        if fused not in (None, True, False):
            raise Exception("QCQPBatch.improve: fused must be None, True or False (fused = %r)" % (fused,))
        if fused is True and not can_fuse:
            raise Exception("QCQPBatch.improve(fused=True): the chain kernel takes n <= %d and at most %d stages (n = %d, %d stages); "
                            "fused=None runs the composed path" % (MAX_N_SMALL, FUSED_MAX_STAGES, self.n, len(stages)))
        if self._suggested is None:
            raise Exception("QCQPBatch.improve: call suggest(RANDOM or SDR, num_samples=R, seed=...) first")
        R, sd, first_index, stride = self._suggested
        if seed is not None and int(seed) != sd:
            raise Exception("QCQPBatch.improve: seed %d differs from the seed of suggest (%d); the batch runs one keyed stream per problem"
                            % (int(seed), sd))
        stats = {}
        rhos = minvs = None
        if any_admm:      # once for every ADMM stage, as _improve_admm does
            m = self.form.m
            if setup == 'device':
                rhos, minvs, lmin, sweeps = self._admm_setup_device(m, rho)
            else:
                rhos = admm_rhos(self.P0s, m, rho)
                minvs, lmin, sweeps = admm_minvs(self.P0s, rhos, m), None, None
            stats = dict(rho=rhos, setup=setup, lambda_min=lmin, setup_sweeps=sweeps)
        E = self.engine
        common = dict(seed=sd, seed_stride=stride, first_index=first_index, cons=self.cons)
        use_fused = can_fuse and fused is not False
        if use_fused:
            code = {s.COORD_DESCENT: E.CHAIN_CD, s.ADMM: E.CHAIN_ADMM}
            out = E.chain_small_batch_run(self.P0s, self.q0s, self.r0s, R, [dict(g, method=code[g['method']]) for g in stages], rhos=rhos,
                                          Minvs=minvs, X0=self._starts, want_x=False, **common)
            per_stage = [dict(d, method=g['method']) for d, g in zip(out['stages'], stages)]
            kernel = E.last_cd_kernel()
        else:
            small = self.n <= MAX_N_SMALL
            X, per_stage, kernels = self._starts, [], []
            for k, g in enumerate(stages):
                want_x = k + 1 < len(stages)      # the points of the last stage are not handed on
                if g['method'] == s.ADMM:
                    run = E.admm_small_batch_run if small else E.admm_batch_run
                    out = run(self.P0s, self.q0s, self.r0s, R, rhos, minvs, X0=X, phase1=g['phase1'], num_iters=g['num_iters'], tol=g['tol'],
                              viol_lim=g['viol_lim'], want_x=want_x, **common)
                    kernels.append(E.last_admm_kernel()[0])
                    keys = E._CHAIN_ADMM_KEYS
                else:
                    run = E.cd_small_batch_run if small else E.cd_batch_run
                    out = run(self.P0s, self.q0s, self.r0s, R, X0=X, phase1=g['phase1'], num_iters=g['num_iters'], viol_tol=g['viol_tol'],
                              tol=g['tol'], want_x=want_x, **common)
                    kernels.append(E.last_cd_kernel())
                    keys = E._CHAIN_CD_KEYS
                X = out['X']
                per_stage.append(dict(((key, out[key]) for key in keys + ('f0', 'maxviol')), method=g['method']))
            kernel = ' + '.join(kernels)
        if stages[-1]['method'] == s.COORD_DESCENT:
            stats['failed_restarts'] = int(np.count_nonzero((out['status1'] != 0) | (out['status2'] != 0)))
        return self._publish(out, [g['method'] for g in stages], R, stages=per_stage, fused=use_fused, kernel=kernel, **stats)

    def close(self):
        self.engine.close()
