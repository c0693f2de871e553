"""The four kernels that rest on the two eigen-solvers (spectral_small_kernel, spectral_wide_kernel, admm_setup_kernel,
admm_setup_wide_kernel) on the lattice of tests/spectrum_cases.py: spectra built exactly, so that the lane-level decisions -- the rank
of an eigen-index among ties, k_min, interior / boundary / hard from the wave sums, the second index per lane past n = 64, the Rayleigh
quotients, the sign rule of q_min, lambda_min + m rho < 0 -- are run on inputs where the right answer is exact and known.

Tier A (a permuted diagonal: the solvers rotate nothing) is judged bit for bit and by the 80-digit reference; Tier B (a dense exact
Q) to ten times the figures that the NumPy restatements reach against that reference on the CPU (spectrum_cases.*_MEASURED).  All
cases of one size go through the C ABI in ONE call per kernel and relop, and every problem of every batch is judged.  Then power-of-two
scaling (exact inside the supported range), the status for a Frobenius norm that underflows or overflows, and a given rho on the two
sides of lambda_min + m rho == 0.  Run with `-m gpu` on an MI355X; the largest figures are printed (profiles/r30_spectrum_lattice.md)."""
from fractions import Fraction

import numpy as np
import pytest

import admm_setup_cases as asc
import spectral_batch_cases as sc
import spectrum_cases as lc

pytestmark = pytest.mark.gpu

KEYS = ('x', 'bound', 'mu', 'lam', 'sweeps', 'branch', 'status')
SETUP_KEYS = ('rho', 'lambda_min', 'Minv', 'sweeps', 'status')
ALL_SIZES = lc.SIZES + lc.SIZES_WIDE
MARGIN = 10.0


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def make(eng_mod, n):
    from qcqp_amd.form import QCQPForm
    return eng_mod.Engine(QCQPForm.from_arrays(lc.boolean_funcs(n)))


def spectral(eng_mod, n, relop, P0s, q0s, r0s, aggs, narrow=False):
    e = make(eng_mod, n)
    call = e.spectral_small_batch if narrow else e.spectral_batch
    o = call(P0s, q0s, r0s, aggs, relop, max_sweeps=lc.MAX_SWEEPS, tol=lc.TOL)
    e.close()
    return o


def setup(eng_mod, n, P0s, **kw):
    e = make(eng_mod, n)
    o = e.admm_batch_setup(P0s, max_sweeps=lc.MAX_SWEEPS, tol=lc.TOL, **kw)
    e.close()
    return o


def same(a, b, keys=KEYS, ia=slice(None), ib=slice(None)):
    return all(np.array_equal(a[k][ia], b[k][ib], equal_nan=True) for k in keys)


# ------------------------------------------------------------------ the spectral kernels
def judge_tier_a(tag, c, relop, n, r):
    lmin = float(np.min(c['lam']))
    want = lc.expected_branch(c, relop)
    assert np.array_equal(r['lam'], np.sort(c['lam'])), tag                       # the sorted diagonal, bit for bit
    assert r['sweeps'] == (0 if n <= 64 else 1), (tag, r['sweeps'])
    assert r['branch'] == want, (tag, r['branch'], want)
    y = lc.y_of(c, r['x'])
    if r['branch'] == 1:
        assert lc.secular_stop_holds(c, r['mu']), (tag, r['mu'])
    if r['branch'] == 2:
        assert Fraction(float(r['mu'])) == -Fraction(lmin), (tag, r['mu'], lmin)
        # q_min is the unit vector of k_min, the LOWEST coordinate that holds lambda_min (rank 0 among the ties), with its one entry
        # positive: that coordinate carries +tau, the other coordinates of the lowest eigenspace carry nothing
        low = np.flatnonzero(np.diag(c['P0']) == lmin)
        e = lc.exact(c['lam'], np.where(c['lam'] == lmin, 0.0, c['gh']), c['rho2'], relop == '==')      # (thr47: the dropped component)
        assert np.all(y[low[1:]] == 0.0), (tag, y[low])
        if e['tau2'] > 0:     # (tau^2 = rho^2 - psi_reg: a tree sum of up to 128 terms, 7 roundings deep, far inside 2^-43 rho^2)
            assert y[low[0]] > 0.0 and abs(y[low[0]] ** 2 - float(e['tau2'])) <= 2.0 ** -43 * c['rho2'], (tag, y[low[0]], e['tau2'])
        else:
            assert y[low[0]] == 0.0, tag


def judge_tier_b(tag, c, relop, r):
    e = lc.exact_case(c, relop)[0]
    lmin = float(np.min(c['lam']))
    got = int(r['branch'])
    if got != e['branch'] and not (relop == '<=' and lmin == 0.0):                # (lambda_min == 0 with <=: the value decides)
        rho = c['rho2'] ** 0.5
        slack = 2.0 ** -40 * (float(np.linalg.norm(c['P0'])) + float(np.linalg.norm(c['g'])) / rho)
        assert e['branch'] == 2 and got == 1 and r['mu'] + lmin <= slack, (tag, got, e['branch'], r['mu'] + lmin, slack)


@pytest.mark.parametrize('relop', ['==', '<='])
@pytest.mark.parametrize('n', ALL_SIZES)
def test_spectral_kernels_on_the_lattice(eng_mod, n, relop):
    from qcqp_amd import sdr
    cs, P0s, q0s, r0s, aggs = lc.batch(n, relop)
    o = spectral(eng_mod, n, relop, P0s, q0s, r0s, aggs)
    if n <= 64:      # the narrow entry point and the wide one make the same launch: the same bits
        assert same(o, spectral(eng_mod, n, relop, P0s, q0s, r0s, aggs, narrow=True))
    cert = sdr.certify_spectral_batch(P0s, q0s, aggs, relop, o['x'], o['mu'])
    worst = dict(lam=0.0, f=0.0, feas=0.0, sweeps=0)
    for b, c in enumerate(cs):                        # every problem: none is left out
        tag = (n, relop, b, lc.case_id(c))
        r = {k: o[k][b] for k in KEYS}
        assert r['status'] == 0, (tag, r['status'], r['sweeps'])
        scale = sc.scale_of(P0s[b], q0s[b], r0s[b], aggs[b])
        assert cert['feasibility'][b] <= 1e-9 * scale and cert['stationarity'][b] <= 1e-9 * scale, (tag, cert['c'][b], cert['stationarity'][b])
        assert cert['lambda_min'][b] >= -1e-9 * scale, (tag, cert['lambda_min'][b])
        if relop == '<=':
            assert r['mu'] >= 0.0 and cert['complementarity'][b] <= 1e-9 * scale, (tag, r['mu'], cert['complementarity'][b])
        if c['tier'] == 'A':
            judge_tier_a(tag, c, relop, n, r)
        else:
            judge_tier_b(tag, c, relop, r)
        if c['rhs'] in lc.THRESHOLD:                  # (the value is continuous across the threshold, to 2^-45 |g| rho: not to rounding)
            continue
        dlam, df, feas = lc.figures(c, relop, r)
        worst = dict(lam=max(worst['lam'], dlam), f=max(worst['f'], df), feas=max(worst['feas'], feas), sweeps=max(worst['sweeps'], int(r['sweeps'])))
        assert dlam <= MARGIN * lc.LAM_MEASURED, (tag, dlam)
        assert df <= MARGIN * lc.F_MEASURED, (tag, df, r['bound'])
        assert feas <= MARGIN * lc.FEAS_MEASURED, (tag, feas)
    print('\nn = %d %s, %d problems: lam %.2e |A|_F, bound %.2e of its scale, feasibility %.2e rho, at most %d sweeps'
          % (n, relop, len(cs), worst['lam'], worst['f'], worst['feas'], worst['sweeps']))


@pytest.mark.parametrize('n', lc.SCALE_SIZES)
def test_power_of_two_scaling_is_exact(eng_mod, n):
    """(P0, q0, r0) times 2^100 and 2^-100, both tiers, both relops: x, sweeps, branch and status bit for bit, lam, mu and bound scaled
    exactly."""
    for relop in ('==', '<='):
        cs, P0s, q0s, r0s, aggs = lc.batch(n, relop)
        base = spectral(eng_mod, n, relop, P0s, q0s, r0s, aggs)
        assert np.all(base['status'] == 0)
        for s in (2.0 ** 100, 2.0 ** -100):
            o = spectral(eng_mod, n, relop, P0s * s, q0s * s, r0s * s, aggs)
            for k in ('x', 'sweeps', 'branch', 'status'):
                assert np.array_equal(o[k], base[k]), (n, relop, s, k)
            for k in ('lam', 'mu', 'bound'):
                assert np.array_equal(o[k], base[k] * s), (n, relop, s, k)


def _degenerate_batch(n, s):
    """[dense Tier B problem times s, diagonal Tier A problem times s, the zero matrix, the dense problem itself]"""
    cs = {(c['tier'], c['spectrum'], c['rhs'], c['cons']): c for c in lc.cases(n, '==')}
    dense, diag = cs['B', 'pm', 'generic', 'bool'], cs['A', 'pm', 'generic', 'bool']
    P0s = np.stack([dense['P0'] * s, diag['P0'] * s, np.zeros((n, n)), dense['P0']])
    q0s = np.stack([dense['q0'] * s, diag['q0'] * s, dense['q0'], dense['q0']])
    return P0s, q0s, np.array([lc.R0 * s, lc.R0 * s, lc.R0, lc.R0]), dense['agg']


@pytest.mark.parametrize('s', [lc.TINY, lc.HUGE], ids=['underflow', 'overflow'])
@pytest.mark.parametrize('n', [33, 66])
def test_a_frobenius_norm_that_underflows_or_overflows_is_status_2(eng_mod, n, s):
    """A matrix with a nonzero entry whose |A|_F^2 evaluates to 0.0 (entries of 2^-600) or to inf (2^520) has no stop test: before
    the fix the narrow solver returned after 0 sweeps with status 0 and a wrong point, and the wide one took its zero-matrix exit.
    Status 2 now, from all four kernels; the zero matrix and an ordinary problem beside them keep status 0 and their bits."""
    P0s, q0s, r0s, agg = _degenerate_batch(n, s)
    alone = spectral(eng_mod, n, '==', P0s[2:], q0s[2:], r0s[2:], agg)
    assert np.array_equal(alone['status'], [0, 0]) and np.all(alone['lam'][0] == 0.0) and alone['sweeps'][0] == 0
    for narrow in ((False, True) if n <= 64 else (False,)):
        o = spectral(eng_mod, n, '==', P0s, q0s, r0s, agg, narrow=narrow)
        assert np.array_equal(o['status'], [2, 2, 0, 0]), (n, s, narrow, o['status'], o['sweeps'])
        assert same(o, alone, ia=slice(2, 4))
    alone = setup(eng_mod, n, P0s[2:])
    assert np.array_equal(alone['status'], [0, 0]) and alone['lambda_min'][0] == 0.0 and alone['rho'][0] == 50.0 * (1.0 / n)
    o = setup(eng_mod, n, P0s)
    assert np.array_equal(o['status'], [2, 2, 0, 0]), (n, s, o['status'], o['sweeps'])
    assert same(o, alone, SETUP_KEYS, ia=slice(2, 4))


# ------------------------------------------------------------------ the setup kernels
@pytest.mark.parametrize('n', ALL_SIZES)
def test_setup_kernels_on_the_lattice(eng_mod, n):
    m = n
    ms = lc.setups(n)
    o = setup(eng_mod, n, np.stack([P0 for _, _, _, _, P0 in ms]))
    assert np.array_equal(o['Minv'], o['Minv'].transpose(0, 2, 1))
    worst = dict(lmin=0.0, minv=0.0)
    for b, (tier, name, Q, lam, P0) in enumerate(ms):
        tag = (n, tier, name)
        lmin, rho, Minv = float(o['lambda_min'][b]), float(o['rho'][b]), o['Minv'][b]
        assert o['status'][b] == 0, (tag, o['status'][b], o['sweeps'][b])
        assert rho == asc.rho_rule(lmin, m), (tag, rho, lmin)                     # the rule applied to what is reported: bit for bit
        if tier == 'A':
            assert lmin == float(lam.min()), (tag, lmin)
            if lam.min() == 0.0:
                assert rho == 50.0 * (1.0 / m), (tag, rho)
            assert np.array_equal(Minv, np.diag(np.diag(Minv))), tag
            want = 1.0 / (2.0 * (np.diag(P0) + rho * m))
            assert np.all(np.abs(np.diag(Minv) - want) <= np.spacing(want)), tag
        else:
            fro = float(np.linalg.norm(P0)) or 1.0      # (n = 1, 'psd0': P0 = 0)
            dl = abs(lmin - float(lam.min())) / fro
            ex = lc.exact_minv(Q, lam, rho, m)
            dm = float(np.max(np.abs(Minv - ex)) / np.max(np.abs(ex)))
            worst = dict(lmin=max(worst['lmin'], dl), minv=max(worst['minv'], dm))
            assert dl <= asc.LMIN_BOUND, (tag, dl)
            assert dm <= MARGIN * lc.MINV_MEASURED, (tag, dm)
    print('\nn = %d, %d setups: lambda_min %.2e |P0|_F, Minv %.2e max |Minv|, at most %d sweeps' % (n, len(ms), worst['lmin'], worst['minv'], int(o['sweeps'].max())))


@pytest.mark.parametrize('n', [4, 64, 128])
def test_a_given_rho_on_the_two_sides_of_the_threshold(eng_mod, n):
    """lambda_min = -2 and m = n: rho = 2 / m (exact at these n) makes lambda_min + m rho == 0 -- NOT status 3, the test is `< 0`; an
    entry of the inverse is 1 / 0, so status 2 --, its next float down makes it negative (status 3, Minv all zero), rho = 3 is
    comfortably above.  Problems 1 and 3 of the batch (lambda_min = -1 and 1) are not affected, bit for bit."""
    P0s, lams = lc.given_rho_batch(n)
    m, on = n, 2.0 / n
    assert on * m == 2.0 and float(np.nextafter(on, 0.0)) * m < 2.0
    for rho, want in ((on, 2), (float(np.nextafter(on, 0.0)), 3), (3.0, 0)):
        o = setup(eng_mod, n, P0s, rho=rho)
        assert np.array_equal(o['status'], [want, 0, want, 0]), (n, rho, o['status'])
        assert np.array_equal(o['rho'], np.full(4, rho)) and np.array_equal(o['lambda_min'], [-2.0, -1.0, -2.0, 1.0])
        for b in (1, 3):
            assert same(o, setup(eng_mod, n, P0s[b:b + 1], rho=rho), SETUP_KEYS, b, 0), (n, rho, b)
        for b in range(4):
            if o['status'][b] == 3:
                assert np.all(o['Minv'][b] == 0.0), (n, rho, b)
            if o['status'][b] == 0:
                ex = lc.exact_minv(np.eye(n), lams[b], rho, m)
                assert np.array_equal(o['Minv'][b], np.diag(np.diag(o['Minv'][b])))
                assert np.all(np.abs(np.diag(o['Minv'][b]) - np.diag(ex)) <= np.spacing(np.diag(ex))), (n, rho, b)
