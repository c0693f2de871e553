"""The multi-launch ADMM path (csrc/admm.h, csrc/gemm_pk.h, csrc/capi_admm.hip) over its dispatch domain, the fused kernel switched
off: every instantiation admm_launch_secular can choose, both tilings of the GEMM, the split planes of both products, both
reductions of the violation -- against a longdouble reference and a derived bound, and against the oracle.

A  qcqpmi_admm_onecons at both sides of every switch of admm_launch_secular (rows 1 .. 8193), nine spectra, bases of signed unit
   vectors (the two products are exact: the secular kernel in isolation) and dense bases at n = 40; real eigenpairs through
   qcqpmi_admm_set_eig at n = 129 and 257, also against the oracle's onecons;
B  the two products as a linear operator x = Q (Q' z) with an arbitrary Q, both GEMM kernels, ragged edges, R = 1; the checker
   refuses a dropped k-block and swapped row blocks;
C  one, two and three iterations of qcqpmi_admm_run, with and without phase 1, every restart against the oracle's improve_admm;
D  admm_apply_constraints, admm_zsolver_device, p0_lambda_min against exact references;
E  refusals.

Not covered: the limit of 16384 basis rows per constraint and the refusal above it (the smallest such basis is 2 GB), the fused
kernel, trajectories longer than three iterations.  Cases, reference and bounds: tests/admm_domain_cases.py (checked on the host
by tests/test_admm_domain_cpu.py); measured figures: profiles/r14_admm_domain.md.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

import admm_domain_cases as ac

pytestmark = pytest.mark.gpu
LD = ac.LD


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def make(eng_mod, funcs, debug=0):
    from qcqp_amd.form import QCQPForm
    e = eng_mod.Engine(QCQPForm.from_arrays(funcs))
    e.admm_fused(False)
    if debug:
        e.L.qcqpmi_debug_profile(e.h, debug << 4, None)
    return e


def worst_ratio(x, ref, bound):
    """max |x - ref| / bound over the elements with a bound; where the bound is zero the device must return ref's bits."""
    err = np.asarray(np.abs(np.asarray(x, dtype=LD) - ref), dtype=np.float64)
    free = bound > 0
    exact_ok = bool(np.all(err[~free] == 0.0))
    return (float(np.max(err[free] / bound[free])) if free.any() else 0.0), exact_ok


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize('case', ac.A_CASES, ids=lambda c: c.id)
def test_onecons_every_secular_instantiation(eng_mod, case):
    """Projection of R = 17 points (two tiles, the second with one column) onto every constraint.  Every element within the derived
    bound of the longdouble reference; coordinates a constraint does not touch (lam = 0 and qhat = 0) and a feasible '<=' point come
    back bit for bit.  Measured worst error / bound per instantiation: profiles/r14_admm_domain.md (at most 0.64)."""
    case.build()
    e = make(eng_mod, case.funcs())
    e.admm_set_basis(case.lam, case.basis(), case.qhat)
    e.upload(case.Z)
    for k in range(case.m):
        x = e.admm_onecons(k + 1)
        ref = case.reference(k)
        w, exact_ok = worst_ratio(x, ref['x'], ref['bound'])
        print('\nA %-40s %-11s k=%d %-8s %-2s worst error / bound %.3f (margin %.1e, cancellation %.1e)' % (
            case.id, case.expected, k + 1, case.kinds[k], case.relop[k], w, ref['margin'], ref['cancel']))
        assert exact_ok, (case.id, k)
        assert np.array_equal(x[ref['untouched']], case.Z[ref['untouched']]), (case.id, k)
        assert w <= 1.0, (case.id, k, w)
    e.close()


@pytest.mark.parametrize('n', ac.A_EIG_NS)
def test_onecons_full_eigenbasis_real_eigenpairs(eng_mod, orc, n):
    """qcqpmi_admm_set_eig (lowrank = 0) with numpy.linalg.eigh pairs of dense indefinite constraints: against the longdouble tier
    (bound) and against the oracle's onecons on the same pairs (both sides float64: the two bounds added)."""
    funcs, lm, Q, Z = ac.eig_problem(n)
    e = make(eng_mod, funcs)
    e.admm_set_eig(lm, Q)
    e.upload(Z)
    prob = orc.Problem(funcs)
    for k in range(len(funcs) - 1):
        x = e.admm_onecons(k + 1)
        ref = ac.eig_reference(funcs, lm, Q, Z, k)
        w, _ = worst_ratio(x, ref['x'], ref['bound'])
        xo = np.stack([prob.onecons(k + 1, Z[:, c], lm[k], Q[k])[0] for c in range(Z.shape[1])], axis=1)
        wo = float(np.max(np.abs(x - xo) / (ref['bound'] + ref['bound_other'])))
        print('\nA set_eig n=%d %s k=%d %s: worst error / bound %.3f against longdouble, %.3f against the oracle (margin %.1e, '
              'cancellation %.1e)' % (n, ac.secular_instantiation(n, False), k + 1, funcs[k + 1][3], w, wo, ref['margin'], ref['cancel']))
        assert w <= 1.0 and wo <= 1.0, (n, k, w, wo)
    e.close()


# ------------------------------------------------------------------------------------------------ B
def test_gemm_checker_refuses_mutants():
    """Host only: a result with one k-block of the second product dropped, and one with the rows of two row blocks swapped."""
    n, m, R = ac.B_CASES[1]
    _, Q, Z = ac.gemm_problem(n, m, R)
    Qk = Q[0]
    good = Qk.dot(Qk.T.dot(Z))
    assert max(ac.gemm_check(good, Qk, Z, ac.sample_columns(R))) <= 1.0
    hat = Qk.T.dot(Z)
    hat[16:32] = 0.0
    swapped = good.copy()
    swapped[0:16], swapped[16:32] = good[16:32], good[0:16]
    for bad in (Qk.dot(hat), swapped):
        assert min(ac.gemm_check(bad, Qk, Z, ac.sample_columns(R))) > 1.0


@pytest.mark.parametrize('n,m,R', ac.B_CASES)
def test_two_products_as_a_linear_operator(eng_mod, n, m, R):
    """lam = 0 supplied, q = 0, r = -1: every point is feasible, the secular kernel hands vhat through bit for bit and onecons returns
    Q_k (Q_k' z) for an arbitrary Q_k.  Bound: (2 gamma_n + gamma_n^2) |Q| |Q'| |z|, nothing else.  Measured: at most 0.022 of it."""
    funcs, Q, Z = ac.gemm_problem(n, m, R)
    g = ac.geometry(n, m, n, False, R)
    e = make(eng_mod, funcs)
    e.admm_set_eig(np.zeros((m, n)), Q)
    e.upload(Z)
    cols = ac.sample_columns(R)
    for k in sorted(set((0, m // 2, m - 1))):
        x = e.admm_onecons(k + 1)
        w_all, w_ld = ac.gemm_check(x, Q[k], Z, cols)
        print('\nB n=%d m=%d R=%d k=%d (%s, %s): worst error / bound %.3f (all columns, float64 reference, 2 x bound), %.3f (%d columns, '
              'longdouble)' % (n, m, R, k + 1, g['gemm1'], g['gemm2'], w_all, w_ld, len(cols)))
        assert w_all <= 1.0 and w_ld <= 1.0
    e.close()


# ------------------------------------------------------------------------------------------------ C
def install(eng_mod, case):
    from qcqp_amd.form import QCQPForm
    form = QCQPForm.from_arrays(case.funcs)
    e = eng_mod.Engine(form)
    e.admm_fused(False)
    if case.debug:
        e.L.qcqpmi_debug_profile(e.h, case.debug << 4, None)
    if case.basis == 'unit':
        e.admm_set_basis(*form.unit_bases())
    elif case.basis == 'full':
        e.admm_set_eig(case.lm, case.Q)
    else:
        e.admm_set_basis(case.lam, case.Bv, case.qhat)
        e.admm_set_bracket(*eng_mod.Engine.reference_bracket(case.lm))
    if case.solver == 'device':
        res, _ = e.admm_zsolver_device(case.rho)
        assert res < 1e-10
    return e


@pytest.mark.parametrize('case', ac.C_CASES, ids=lambda c: c.id)
def test_one_to_three_iterations_against_the_oracle(eng_mod, orc, case):
    """num_iters = 1, 2, 3, phase 1 on and off: every restart within 1e-9 (1 + |x|) of the oracle's improve_admm on the same
    eigenpairs, the iteration counts those of the oracle's trajectory (ac.oracle_admm), the reported f0 / maxviol those of
    Engine.eval().  Measured worst deviation over all cases: 6.0e-14 (profiles/r14_admm_domain.md)."""
    from conftest import oracle_map
    case.build()
    e = install(eng_mod, case)
    prob = orc.Problem(case.funcs)
    prob._eig = (case.lm, case.Q)
    R = case.R
    worst, left, stayed = 0.0, False, False
    for p1 in (True, False):
        for iters in ac.C_ITERS:
            e.upload(case.X0)
            out = e.admm_run(case.rho, case.Minv, phase1=p1, num_iters=iters, viol_lim=case.viol_lim)
            assert e.last_admm_kernel()[0] == ('admm_multi_launch<unit bases>' if case.basis == 'unit' else 'admm_multi_launch')
            X = e.download()
            f0, mv = e.eval()
            assert np.max(np.abs(out['f0'] - f0) / (1 + np.abs(f0))) < 1e-9 and np.max(np.abs(out['maxviol'] - mv)) < 1e-9
            res = oracle_map(lambda r: ac.oracle_admm(prob, case.X0[:, r], case.rho, iters, p1, case.viol_lim), range(R))
            Xo = np.stack([t[0] for t in res], axis=1)
            dev = float(np.max(np.abs(X - Xo) / (1 + np.abs(Xo))))
            worst = max(worst, dev)
            i1, i2 = np.array([t[1] for t in res]), np.array([t[2] for t in res])
            print('\nC %-22s phase1=%d iters=%d: worst deviation %.2e; iters1 %s iters2 %s' % (case.id, p1, iters, dev,
                                                                                             sorted(set(out['iters1'].tolist())), sorted(set(out['iters2'].tolist()))))
            assert dev < ac.C_TOL, (case.id, p1, iters, dev)
            assert np.array_equal(out['iters1'], i1), (case.id, p1, iters, out['iters1'], i1)
            assert np.array_equal(out['iters2'], i2), (case.id, p1, iters, out['iters2'], i2)
            if case.feasible_starts and p1:
                assert np.all(out['iters1'][case.feasible_cols] == 0) and np.any(out['iters1'] > 0)
            left, stayed = left or bool(np.any(out['iters2'] < iters)), stayed or bool(np.any(out['iters2'] == iters))
    if case.viol_lim < 1e4:
        assert left and stayed                             # some restarts leave phase 2 through viol_lim, some stay
    if case.feasible_starts:
        # viol_lim below zero ends phase 2 at its first iteration before anything is taken: what comes back is better(x0, z1) of phase 1,
        # and a restart that was feasible at the start never left x0 -- bit for bit, whatever its tile neighbours did meanwhile
        e.upload(case.X0)
        out = e.admm_run(case.rho, case.Minv, phase1=True, num_iters=3, viol_lim=-1.0)
        X = e.download()
        assert np.array_equal(X[:, case.feasible_cols], case.X0[:, case.feasible_cols])
        assert np.all(out['iters1'][case.feasible_cols] == 0) and np.all(out['iters2'] == 0)
        moved = np.setdiff1d(np.arange(R), case.feasible_cols)
        assert np.any(out['iters1'][moved] > 0) and not np.array_equal(X[:, moved], case.X0[:, moved])
    print('C %-22s worst over 6 runs %.2e' % (case.id, worst))
    e.close()


# ------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize('n', ac.APPLY_NS)
@pytest.mark.parametrize('p', ac.APPLY_PS)
def test_apply_constraints(eng_mod, n, p):
    """out[k] = P_k V (shared) and P_k V_k: longdouble reference, bound gamma_(ceil(n / 2) + 1) |P| |V|."""
    funcs, _, _, _ = ac.eig_problem(n, m=3, seed=p)
    e = make(eng_mod, funcs)
    P = np.stack([f[0] for f in funcs[1:]])
    rs = np.random.RandomState(100 * n + p)
    for shared in (True, False):
        V = rs.randn(n, p) if shared else rs.randn(3, n, p)
        out = e.admm_apply_constraints(V, shared=shared)
        Pl, Vl = np.asarray(P, dtype=LD), np.asarray(V, dtype=LD)
        ref = np.stack([Pl[k].dot(Vl if shared else Vl[k]) for k in range(3)])
        w, _ = worst_ratio(out, ref, ac.apply_bound(P, V))
        print('\nD apply_constraints n=%d p=%d shared=%d: worst error / bound %.3f' % (n, p, shared, w))
        assert w <= 1.0
    e.close()


@pytest.mark.parametrize('n', ac.ZSOLVER_NS)
def test_zsolver_device_inverse(eng_mod, n):
    """(2 (P0 + rho m I))^-1 by Newton-Schulz, read back THROUGH the iteration: m = 1, rho = 1 / 2, q0 = 0 and a constraint that every
    point satisfies make the first phase-2 iterate z = Minv x0 with x0 = I -- one nonzero product per entry, exact --, and z (the
    minimiser of f0 + rho |z - x0|^2) is strictly better than x0, so admm_run leaves it in the population.  Checked: the documented
    residual max |M X - I| < 1e-10 in longdouble, and every entry against an inverse good to 2^-64 (ac.inverse_yardstick).
    Bound: the refinement step X + X R with R = I - M X in double-double gives M^-1 (I - R^2) exactly, then rounds once:
    1.01 u |M^-1_ij| + ||M^-1||_inf ||R||_inf^2, where the float64 Newton-Schulz iterate it starts from has
    ||R||_inf <= n16^2 res (the exact step squares the previous residual, res = its reported estimate, a maximum over entries)
    + 3 gamma_n16 t^2, t = || |M| |M^-1| ||_inf (the roundings of T = M X, U = X T and 2 X - U, multiplied by M)."""
    rs = np.random.RandomState(n)
    A = rs.randn(n, n)
    P0 = A.T.dot(A) / n + 0.25 * np.eye(n)
    P0 = (P0 + P0.T) / 2.
    funcs = [(P0, np.zeros(n), 0.0, None), (np.zeros((n, n)), np.concatenate([[1.0], np.zeros(n - 1)]), -1e6, '<=')]
    e = make(eng_mod, funcs)
    rho = 0.5
    lam, Bv, qhat = np.zeros((1, 1)), np.zeros((1, 1, n)), np.ones((1, 1))
    Bv[0, 0, 0] = 1.0
    e.admm_set_basis(lam, Bv, qhat)
    res, its = e.admm_zsolver_device(rho)
    assert res < 1e-10, (res, its)
    e.upload(np.eye(n))
    out = e.admm_run(rho, None, phase1=False, num_iters=1)
    assert np.all(out['iters2'] == 1)
    X = e.download()                                     # column j = Minv e_j
    M64 = 2. * (P0 + rho * np.eye(n))
    M = np.asarray(M64, dtype=LD)
    resid = float(np.max(np.abs(M.dot(np.asarray(X, dtype=LD)) - np.eye(n))))
    Ml, _ = ac.inverse_yardstick(M64)
    Minv = np.asarray(Ml, dtype=np.float64)
    n16 = ac.n16_of(n)
    t = float(np.abs(M64).dot(np.abs(Minv)).sum(axis=1).max())
    floor = n16 ** 2 * res + 3 * ac.gamma(n16) * t * t
    bound = 1.01 * ac.U * np.abs(Minv) + float(np.abs(Minv).sum(axis=1).max()) * floor ** 2 + 4 * ac.ULD * np.abs(Minv)
    w, _ = worst_ratio(X, Ml, bound)
    print('\nD zsolver_device n=%d: %d iterations, residual estimate %.1e, max |M X - I| %.2e, worst entry error / bound %.3f' % (n, its, res, resid, w))
    assert resid < 1e-10
    assert w <= 1.0
    e.close()


@pytest.mark.parametrize('kind', ['diag', 'dense'])
def test_p0_lambda_min(eng_mod, kind):
    n = 37
    rs = np.random.RandomState(5)
    if kind == 'diag':
        import scipy.sparse as sp
        d = rs.randn(n)
        P0, ev = sp.diags(d, format='csr'), np.sort(d)
    else:
        A = rs.randn(n, n)
        P0 = (A + A.T) / 2.
        ev = np.linalg.eigvalsh(P0)
    funcs = [(P0, np.zeros(n), 0.0, None), (np.eye(n), np.zeros(n), -1.0, '<=')]
    e = make(eng_mod, funcs)
    lmin, steps = e.p0_lambda_min()
    print('\nD p0_lambda_min %s: %.15g against %.15g after %d steps' % (kind, lmin, ev[0], steps))
    assert ev[0] < 0 and abs(lmin - ev[0]) <= 1e-9 * max(1.0, np.abs(ev).max())
    if kind == 'diag':
        assert lmin == ev[0] and steps == 0
    e.close()


# ------------------------------------------------------------------------------------------------ E
def test_refusals(eng_mod):
    from qcqp_amd.engine import EngineError
    n, m = 12, 2
    rs = np.random.RandomState(0)
    A = rs.randn(n, n)
    P0 = A.T.dot(A) + np.eye(n)
    funcs = [(P0, np.zeros(n), 0.0, None)] + [(np.eye(n), rs.randn(n), -1.0, '<=') for _ in range(m)]
    e = make(eng_mod, funcs)
    e.upload(rs.randn(n, 5))

    def refused(fn, *a, **kw):
        with pytest.raises(EngineError) as ei:
            fn(*a, **kw)
        return ei.value.code

    EINVAL, ESTATE, EUNSUPPORTED = -1, -3, -4                                           # include/qcqp_mi.h
    assert refused(e.admm_run, 1.0, np.eye(n)) == ESTATE                                # before any setup
    assert refused(e.admm_set_bracket, -np.ones(m), np.ones(m)) == ESTATE               # before a basis
    assert refused(e.admm_onecons, 1) == ESTATE
    for rp in (3, 5, 6, 7):
        assert refused(e.admm_set_basis, np.zeros((m, rp)), np.zeros((m, rp, n)), np.zeros((m, rp))) == EUNSUPPORTED, rp
    assert refused(e.admm_set_basis, np.zeros((m, n + 1)), np.zeros((m, n + 1, n)), np.zeros((m, n + 1))) == EINVAL      # rp > n
    B = np.zeros((m, 2, n)); B[:, 0, 0] = 1.0; B[:, 1, 1] = 1.0
    e.admm_set_basis(np.ones((m, 2)), B, np.zeros((m, 2)))
    assert refused(e.admm_set_bracket, np.array([0.5, -1.0]), np.ones(m)) == EINVAL   # slo > 0
    assert refused(e.admm_set_bracket, -np.ones(m), np.array([1.0, -0.5])) == EINVAL  # ehi < 0
    e.admm_set_bracket(-np.ones(m), np.ones(m))
    assert refused(e.admm_onecons, 0) == EINVAL
    assert refused(e.admm_onecons, m + 1) == EINVAL
    assert e.admm_onecons(m).shape == (n, 5)
    assert refused(e.admm_run, 1.0, None) == EINVAL                                    # dense P0 and no Minv
    e.close()
