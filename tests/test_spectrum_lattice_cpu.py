"""The lattice of tests/spectrum_cases.py on the CPU: that its matrices ARE what they claim (rational arithmetic), that its reference
agrees with an independent solver, and that the NumPy restatements of the four eigen-solver kernels stay within the constants that
tests/test_gpu_spectrum_lattice.py allows the kernels ten times of.  The eigen-solvers are run once per matrix (a memo around
spectral_batch_cases.jacobi and spectral_wide_cases.jacobi_wide: every right-hand side of a matrix shares its decomposition); past
n = 64 a fixed subset is restated (WIDE_RESTATED), so that the file stays well under a minute."""
import warnings
from fractions import Fraction

import numpy as np
import pytest

import admm_setup_cases as asc
import spectral_batch_cases as sc
import spectral_wide_cases as wc
import spectrum_cases as lc

ALL_SIZES = lc.SIZES + lc.SIZES_WIDE
WIDE_RESTATED = (65, 128)
SCALED = (33, 65)


@pytest.fixture(scope='module', autouse=True)
def one_decomposition_per_matrix():
    memo, narrow, wide = {}, sc.jacobi, wc.jacobi_wide

    def cached(fn, name):
        def run(A, max_sweeps=sc.MAX_SWEEPS, tol=sc.TOL):
            key = (name, A.shape, A.tobytes(), max_sweeps, tol)
            if key not in memo:
                memo[key] = fn(A, max_sweeps, tol)
            return memo[key]
        return run

    sc.jacobi, wc.jacobi_wide = cached(narrow, 'narrow'), cached(wide, 'wide')
    yield
    sc.jacobi, wc.jacobi_wide = narrow, wide


def restate(c, relop, scale=1.0):
    fn = sc.restate if c['lam'].size <= 64 else wc.restate
    return fn(c['P0'] * scale, c['q0'] * scale, c['r0'] * scale, c['agg'], relop, max_sweeps=lc.MAX_SWEEPS, tol=lc.TOL)


@pytest.mark.parametrize('n', ALL_SIZES)
def test_the_lattice_is_exact(n):
    """Q'Q == I in double arithmetic; P0 == Q diag(lam) Q' and g == Q gh entry for entry, as rationals; for the box 0.5 q0 - P0 h == g;
    the spectra keep max |lam| / min nonzero |lam| <= 2^12."""
    for (tier, name), (Q, lam, P0) in lc.matrices(n).items():
        assert np.array_equal(Q.T.dot(Q), np.eye(n)) and np.array_equal(Q.dot(Q.T), np.eye(n)), (tier, name)
        if tier == 'A':
            assert np.array_equal(np.sort(Q, axis=0)[-1], np.ones(n)) and np.count_nonzero(Q) == n
        elif n >= 4:
            assert np.count_nonzero(Q) > 4 * n or n < 16, 'a dense Q'
        nz = np.abs(lam[lam != 0.0])
        assert nz.size == 0 or nz.max() / nz.min() <= 2.0 ** 12
        rat = lc.rational_p0(Q, lam)
        assert all(Fraction(float(P0[i, j])) == rat[i, j] for i in range(n) for j in range(n)), (tier, name)
        rows = [sum(rat[i]) for i in range(n)]
        Qi = np.rint(Q * 64.0).astype(np.int64)
        for relop in ('==', '<='):
            for c in lc.cases(n, relop):
                if (c['tier'], c['spectrum']) != (tier, name):
                    continue
                if tier == 'A':
                    assert np.array_equal(c['g'][np.argmax(Q, axis=0)], c['gh']), lc.case_id(c)
                else:
                    gi = Qi.dot(c['gh'].astype(np.int64))
                    assert np.array_equal(c['gh'], np.rint(c['gh'])) and all(Fraction(float(v)) == Fraction(int(w), 64) for v, w in zip(c['g'], gi))
                if c['cons'] == 'box':      # h = -1/2: 0.5 q0 - P0 h = 0.5 (q0 + P0 1)
                    assert all((Fraction(float(q)) + r) / 2 == Fraction(float(g)) for q, r, g in zip(c['q0'], rows, c['g'])), lc.case_id(c)
                else:
                    assert np.array_equal(c['q0'], 2.0 * c['g'])


@pytest.mark.parametrize('n', ALL_SIZES)
def test_exact_agrees_with_the_independent_solver(n):
    worst = 0.0
    for relop in ('==', '<='):
        for c in lc.cases(n, relop):
            if c['rhs'] != 'generic':
                continue
            e, opt = lc.exact_case(c, relop)
            ind = sc.independent(c['P0'], c['q0'], c['r0'], c['agg'], relop)
            df = float(abs(Fraction(float(ind['bound'])) - opt)) / lc.f_scale(c)
            worst = max(worst, df)
            assert ind['branch'] == e['branch'] and df <= lc.INDEPENDENT_RTOL, (n, relop, lc.case_id(c), ind['branch'], e['branch'], df)
            if e['branch'] == 1:
                assert abs(ind['mu'] - float(e['mu'])) <= 1e-9 * (1.0 + abs(float(e['mu']))), (n, relop, lc.case_id(c))
    print('\nn = %d: independent against exact, %.2e of the scale' % (n, worst))


@pytest.mark.parametrize('n', lc.SIZES + WIDE_RESTATED)
def test_restatements_stay_within_the_measured_constants(n):
    worst = dict(lam=0.0, f=0.0, feas=0.0, minv=0.0, lmin=0.0)
    for relop in ('==', '<='):
        for c in lc.cases(n, relop):
            tag = (n, relop, lc.case_id(c))
            r = restate(c, relop)
            e = lc.exact_case(c, relop)[0]
            lmin = float(np.min(c['lam']))
            assert r['status'] == 0, (tag, r['status'], r['sweeps'])
            if c['tier'] == 'A':                  # what the GPU test asks of the kernels, bit for bit
                assert r['sweeps'] == (0 if n <= 64 else 1) and np.array_equal(r['lam'], np.sort(c['lam'])), tag
                assert r['branch'] == lc.expected_branch(c, relop), (tag, r['branch'])
                if r['branch'] == 1:
                    assert lc.secular_stop_holds(c, r['mu']), (tag, r['mu'])
                if r['branch'] == 2:
                    assert Fraction(float(r['mu'])) == -Fraction(lmin), tag
            elif r['branch'] != e['branch'] and not (relop == '<=' and lmin == 0.0):
                slack = 2.0 ** -40 * (float(np.linalg.norm(c['P0'])) + float(np.linalg.norm(c['g'])) / c['rho2'] ** 0.5)
                assert e['branch'] == 2 and r['branch'] == 1 and r['mu'] + lmin <= slack, (tag, r['branch'], e['branch'], r['mu'] + lmin)
            if c['rhs'] in lc.THRESHOLD:
                continue
            dlam, df, feas = lc.figures(c, relop, r)
            worst.update(lam=max(worst['lam'], dlam), f=max(worst['f'], df), feas=max(worst['feas'], feas))
            assert dlam <= lc.LAM_MEASURED and df <= lc.F_MEASURED and feas <= lc.FEAS_MEASURED, (tag, dlam, df, feas)
    for tier, name, Q, lam, P0 in lc.setups(n):
        r = asc.restate(P0, n, max_sweeps=lc.MAX_SWEEPS, tol=lc.TOL)
        assert r['status'] == 0 and r['rho'] == asc.rho_rule(r['lambda_min'], n), (n, tier, name)
        ex = lc.exact_minv(Q, lam, r['rho'], n)
        dm = float(np.max(np.abs(r['Minv'] - ex)) / np.max(np.abs(ex)))
        dl = abs(r['lambda_min'] - float(lam.min())) / (float(np.linalg.norm(P0)) or 1.0)      # (n = 1, 'psd0': P0 = 0)
        worst.update(minv=max(worst['minv'], dm), lmin=max(worst['lmin'], dl))
        assert dm <= lc.MINV_MEASURED and dl <= asc.LMIN_MEASURED, (n, tier, name, dm, dl)
        if tier == 'A':
            assert r['lambda_min'] == float(lam.min()) and np.array_equal(r['Minv'], np.diag(np.diag(r['Minv']))), (n, name)
    print('\nn = %d: %s' % (n, ', '.join('%s %.2e' % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize('n', SCALED)
def test_power_of_two_scaling_of_the_restatements_is_exact(n):
    for relop in ('==', '<='):
        for c in lc.cases(n, relop):
            if c['rhs'] not in ('generic', 'zeroL'):
                continue
            base = restate(c, relop)
            for s in (2.0 ** 100, 2.0 ** -100):
                r = restate(c, relop, s)
                tag = (n, relop, lc.case_id(c), s)
                assert np.array_equal(r['x'], base['x']) and (r['sweeps'], r['branch'], r['status']) == (base['sweeps'], base['branch'], base['status']), tag
                assert np.array_equal(r['lam'], base['lam'] * s) and r['mu'] == base['mu'] * s and r['bound'] == base['bound'] * s, tag


@pytest.mark.parametrize('n', [33, 66])
def test_a_degenerate_frobenius_norm_is_status_2_in_the_restatements(n):
    """The mirror of JacobiResult::degenerate / JacobiWideResult::degenerate: entries of 2^-600 (every square underflows) and of 2^520
    (they overflow) give status 2 from the three restatements; the zero matrix and the matrix itself keep status 0."""
    c = [c for c in lc.cases(n, '==') if lc.case_id(c) == 'B-pm-generic-bool'][0]
    zero = dict(c, P0=np.zeros((n, n)))
    assert restate(c, '==')['status'] == 0 and restate(zero, '==')['status'] == 0
    assert asc.restate(c['P0'], n, max_sweeps=lc.MAX_SWEEPS)['status'] == 0 and asc.restate(zero['P0'], n)['status'] == 0
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        for s in (lc.TINY, lc.HUGE):
            sq = (c['P0'][c['P0'] != 0.0] * s) ** 2
            assert np.all(sq == 0.0) if s < 1.0 else np.max(sq) == np.inf
            assert restate(c, '==', s)['status'] == 2, (n, s)
            assert asc.restate(c['P0'] * s, n, max_sweeps=lc.MAX_SWEEPS)['status'] == 2, (n, s)
            assert asc.restate(np.diag(np.diag(c['P0'])) * s, n)['status'] == 2, (n, s)
    assert (sc.degenerate_norm if n <= 64 else wc.degenerate_norm)(c['P0'] * lc.TINY)
    assert not (sc.degenerate_norm if n <= 64 else wc.degenerate_norm)(c['P0'] * 2.0 ** -100)
