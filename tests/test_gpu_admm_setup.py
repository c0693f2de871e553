"""qcqpmi_admm_batch_setup / Engine.admm_batch_setup / QCQPBatch.improve(ADMM, setup='device'): rho_b by the reference's rule and
Minv_b = (2 (P0_b + rho_b m I))^-1 for B small problems from ONE eigendecomposition each in ONE launch of admm_setup_kernel (n <= 64) or
admm_setup_wide_kernel (65 <= n <= 128) (csrc/admm_setup.h).

The grid is that of tests/admm_setup_cases.py, on which tests/test_setup_grid_cpu.py holds the NumPy restatement to the same
statements: the sizes are the smallest at which each kernel can go wrong (1 padded to 2, odd and even around half and full wave; one,
two and 64 live lanes in slot 1), the families put lambda_min on both sides of the rule's branch and exactly on it.  Then what does
not depend on the last bit -- a problem's result against itself under every change of its surroundings, bit for bit --, a given rho,
the ADMM launch fed from the device setup against the oracle at the horizon of admm_batch_cases, the facade, and the refusals."""
import numpy as np
import pytest

import admm_batch_cases as ab
import admm_setup_cases as asc
import admm_wide_cases as aw
from conftest import oracle_map

pytestmark = pytest.mark.gpu

KEYS = ('rho', 'lambda_min', 'Minv', 'sweeps', 'status')


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def make(eng_mod, funcs):
    from qcqp_amd.form import QCQPForm
    return eng_mod.Engine(QCQPForm.from_arrays(funcs))


def setup(eng_mod, funcs, P0s, **kw):
    """One call on a context built from `funcs` (its constraints give n and m)."""
    e = make(eng_mod, funcs)
    o = e.admm_batch_setup(P0s, **kw)
    e.close()
    return o


def same(a, b, ia=slice(None), ib=slice(None)):
    return all(np.array_equal(a[k][ia], b[k][ib]) for k in KEYS)


@pytest.mark.parametrize('c', asc.cases(), ids=asc.case_id)
def test_setup_against_the_host_and_the_oracle(eng_mod, orc, c):
    name, n, B = c
    fl = asc.family(name, n, B)
    P0s = asc.sc.objectives(fl)[0]
    m = len(fl[0]) - 1
    o = setup(eng_mod, fl[0], P0s)
    assert np.array_equal(o['Minv'], o['Minv'].transpose(0, 2, 1))
    rs = np.random.RandomState(n)
    worst = 0.0
    for b in range(B):
        r = asc.restated(name, n, b)
        fro, ref = float(np.linalg.norm(P0s[b])), float(np.linalg.eigvalsh(P0s[b])[0])
        assert o['status'][b] == 0 and abs(int(o['sweeps'][b]) - r['sweeps']) <= 2, (b, o['status'][b], o['sweeps'][b], r['sweeps'])
        dev = abs(o['lambda_min'][b] - ref)
        worst = max(worst, dev / fro if fro else dev)
        assert dev <= asc.LMIN_BOUND * fro, (b, dev, fro)
        assert o['rho'][b] == asc.rho_rule(float(o['lambda_min'][b]), m)          # the rule applied to what is reported: bit for bit
        auto = orc.Problem(fl[b]).auto_rho()
        if abs(ref) > asc.LMIN_GATE * fro:
            assert abs(o['rho'][b] - auto) <= asc.RHO_RTOL * auto, (b, o['rho'][b], auto)
        else:
            assert fro == 0.0                                                    # on this grid only P0 = 0 sits on the rule's jump
        if fro == 0.0:
            # (50 / m in the rule's own order of operations, 50 * (1 / m): the bits of admm_rhos, within an ulp of the quotient)
            assert o['lambda_min'][b] == 0.0 and o['rho'][b] == 50.0 * (1.0 / m) == auto and abs(o['rho'][b] - 50.0 / m) <= np.spacing(50.0 / m)
            want = np.eye(n) / (2.0 * o['rho'][b] * m)
            assert np.all(np.abs(o['Minv'][b] - want) <= np.spacing(want))
        if name == 'diag':                                                       # eigenvalues found exactly: the host's bits
            from qcqp_amd import batch
            assert o['rho'][b] == batch.admm_rhos(P0s[b:b + 1], m)[0]
        rhs = rs.randn(n)
        assert ab.rel(o['Minv'][b].dot(rhs), asc.cholesky_solve(P0s[b], auto, m, rhs)) <= asc.SOLVE_RTOL, b
    print('\n%s: lambda_min within %.1e |P0|_F of eigvalsh (bound %.1e)' % (asc.case_id(c), worst, asc.LMIN_BOUND))


def _random_symmetric(B, n, seed):
    M = np.random.RandomState(seed).randn(B, n, n)
    return 0.5 * (M + M.transpose(0, 2, 1))


@pytest.mark.parametrize('name,n', [('cut', 33), ('bls', 96)])
def test_a_problem_depends_on_its_own_data_alone(eng_mod, name, n):
    """B = 1 against the same problem inside B = 5 at another position, and a reversed batch."""
    fl = asc.family(name, n, 5)
    P0s = asc.sc.objectives(fl)[0]
    o = setup(eng_mod, fl[0], P0s)
    assert (o['status'] == 0).all()
    for b in (0, 3):
        o1 = setup(eng_mod, fl[0], P0s[b:b + 1])
        assert same(o, o1, b, 0), b
    moved = setup(eng_mod, fl[0], P0s[[3, 4, 0, 1, 2]])
    assert same(o, moved, 3, 0) and same(o, moved, 0, 2)
    assert same(o, setup(eng_mod, fl[0], P0s[::-1]), slice(None), slice(None, None, -1))


@pytest.mark.parametrize('n,B', [(4, 20000), (65, 2500)])
def test_more_problems_than_resident_workgroups(eng_mod, n, B):
    """The ticket loop: B = 20000 at n = 4 for the narrow kernel, B = 2500 at n = 65 (84 MB of output) for the wide one.  Every
    problem is the problem of the reversed batch, and three of them are the batch of one, bit for bit."""
    funcs = asc.family('bls', n, 1)[0]
    P0s = _random_symmetric(B, n, 5)
    o = setup(eng_mod, funcs, P0s)
    assert (o['status'] == 0).all()
    assert np.array_equal(o['Minv'], o['Minv'].transpose(0, 2, 1))
    assert same(o, setup(eng_mod, funcs, np.ascontiguousarray(P0s[::-1])), slice(None), slice(None, None, -1))
    for b in (0, B // 2 + 1, B - 1):
        assert same(o, setup(eng_mod, funcs, P0s[b:b + 1]), b, 0), b
    lmin = np.linalg.eigvalsh(P0s)[:, 0]
    assert np.max(np.abs(o['lambda_min'] - lmin) / np.linalg.norm(P0s, axis=(1, 2))) <= asc.LMIN_BOUND


@pytest.mark.parametrize('n', [16, 66])
def test_given_rho(eng_mod, n):
    fl, P0s, m, rho_ok, rho_small, lmin = asc.given_rho_case(n)
    o = setup(eng_mod, fl[0], P0s, rho=rho_ok)
    assert (o['status'] == 0).all() and np.array_equal(o['rho'], np.full(3, rho_ok))
    assert np.array_equal(o['Minv'], o['Minv'].transpose(0, 2, 1))
    from qcqp_amd import batch
    host = batch.admm_minvs(P0s, o['rho'], m)
    assert np.max(np.abs(o['Minv'] - host)) <= 1e-12 * np.max(np.abs(host))
    short = lmin + m * rho_small < 0
    assert short.any() and not short.all()
    o = setup(eng_mod, fl[0], P0s, rho=rho_small)
    assert np.array_equal(o['status'], np.where(short, 3, 0)) and np.array_equal(o['rho'], np.full(3, rho_small))
    for b in range(3):
        o1 = setup(eng_mod, fl[0], P0s[b:b + 1], rho=rho_small)
        assert same(o, o1, b, 0), b                              # the others are not affected by a neighbour that fails
        assert np.any(o['Minv'][b] != 0.0) != bool(short[b])    # and a problem that fails has no inverse


def _run_cases():
    return ([c for c in ab.cases() if c[1] in (7, 33, 64)] + [c for c in aw.cases() if c[1] in (65, 96, 128)])


@pytest.mark.parametrize('c', _run_cases(), ids=ab.case_id)
def test_run_accepts_the_device_setup(eng_mod, orc, c):
    """rhos and Minvs of admm_batch_setup go into admm_batch_run at NUM_ITERS = 5 per phase; every restart against the oracle's
    improve_admm from the same start with the same rho, both iteration counts equal and point, objective and violation to PARITY =
    1e-9.  Why that should hold: the device inverse differs from the host's by about 1e-14 relative and the iteration at most doubles
    a difference per step, which leaves about 1e-11 after ten steps (derived, not measured; the worst value is printed)."""
    name, n, B, R, ps, seed, stride, fi = c
    fl = ab.family(name, n, B, seed=ps)
    P0s, q0s, r0s = ab.objectives(fl)
    m = len(fl[0]) - 1
    e = make(eng_mod, fl[0])
    s = e.admm_batch_setup(P0s)
    assert (s['status'] == 0).all()
    o = e.admm_batch_run(P0s, q0s, r0s, R, s['rho'], s['Minv'], seed=seed, seed_stride=stride, first_index=fi, num_iters=ab.NUM_ITERS)
    kernel = e.last_admm_kernel()[0]
    e.close()
    assert kernel == 'admm_small_kernel<%d%s>' % (4 if name in ab.MAXC4 else 1, ',w2' if n > 64 else '')
    for b in range(B):
        lm = float(np.linalg.eigvalsh(P0s[b])[0])
        if abs(lm) > asc.LMIN_GATE * np.linalg.norm(P0s[b]):
            auto = orc.Problem(fl[b]).auto_rho()
            assert abs(s['rho'][b] - auto) <= asc.RHO_RTOL * auto, (b, s['rho'][b], auto)
    X0 = ab.starts(orc, seed, stride, fi, B, R, n)
    X, i1, i2, f, v = ab.oracle_batch(orc, oracle_map, fl, X0, rhos=s['rho'], num_iters=ab.NUM_ITERS)
    dev = max(ab.rel(o['X'][b, r], X[b, r]) for b in range(B) for r in range(R))
    df = float(np.max(np.abs(o['f0'] - f) / (1.0 + np.abs(f))))
    dv = float(np.max(np.abs(o['maxviol'] - v)))
    print('\n%s: %d restarts from the device setup, point %.1e, f0 %.1e, max violation %.1e' % (ab.case_id(c), B * R, dev, df, dv))
    assert np.array_equal(o['iters1'], i1) and np.array_equal(o['iters2'], i2)
    assert dev < ab.PARITY and df < ab.PARITY and dv < ab.PARITY, (dev, df, dv)


@pytest.mark.parametrize('n,wide', [(33, False), (96, True)])
def test_facade(eng_mod, n, wide):
    from qcqp_amd import settings as s
    from qcqp_amd.batch import QCQPBatch
    B, R, seed = 3, 5, 17
    fl = ab.family('bls', n, B, seed=2)
    got = {}
    for label, kw in (('plain', {}), ('host', dict(setup='host')), ('device', dict(setup='device'))):
        qb = QCQPBatch(fl)
        qb.suggest(s.RANDOM, num_samples=R, seed=seed)
        if label == 'plain':
            with pytest.raises(Exception, match="setup must be 'host' or 'device'"):
                qb.improve(s.ADMM, num_iters=5, wide=wide, setup='gpu')
            assert qb.last_stats is None and qb.engine.last_admm_kernel()[0] == ''      # before any launch
        f, v = qb.improve(s.ADMM, num_iters=5, wide=wide, **kw)
        got[label] = dict(f=f, v=v, x=qb.x, best_index=qb.best_index, pf=qb.population_f, pv=qb.population_v, stats=qb.last_stats)
        qb.close()
    # the default call is the call with setup='host': results and last_stats, bit for bit
    for k in ('f', 'v', 'x', 'best_index', 'pf', 'pv'):
        assert np.array_equal(got['plain'][k], got['host'][k]), k
    assert set(got['plain']['stats']) == set(got['host']['stats'])
    for k, val in got['plain']['stats'].items():
        other = got['host']['stats'][k]
        assert (val is None and other is None) or np.array_equal(val, other), k
    assert got['host']['stats']['setup'] == 'host' and got['host']['stats']['lambda_min'] is None
    # the device setup: the same winners and counts, the values to PARITY
    h, d = got['host'], got['device']
    assert d['stats']['setup'] == 'device' and d['stats']['kernel'] == h['stats']['kernel']
    assert np.array_equal(d['best_index'], h['best_index'])
    assert np.array_equal(d['stats']['iters1'], h['stats']['iters1']) and np.array_equal(d['stats']['iters2'], h['stats']['iters2'])
    for k in ('f', 'v', 'x', 'pf', 'pv'):
        assert ab.rel(d[k], h[k]) <= ab.PARITY, (k, ab.rel(d[k], h[k]))
    assert ab.rel(d['stats']['rho'], h['stats']['rho']) <= asc.RHO_RTOL
    lmin = np.linalg.eigvalsh(ab.objectives(fl)[0])[:, 0]
    assert np.max(np.abs(d['stats']['lambda_min'] - lmin)) <= asc.LMIN_BOUND * np.max(np.linalg.norm(ab.objectives(fl)[0], axis=(1, 2)))
    assert d['stats']['setup_sweeps'].shape == (B,) and (d['stats']['setup_sweeps'] >= 1).all()


def test_facade_words_a_small_rho_as_the_host_path_does(eng_mod):
    from qcqp_amd import settings as s
    from qcqp_amd.batch import QCQPBatch
    fl, P0s, m, rho_ok, rho_small, lmin = asc.given_rho_case()
    text = {}
    for setup_ in ('host', 'device'):
        qb = QCQPBatch(fl)
        qb.suggest(s.RANDOM, num_samples=2, seed=3)
        with pytest.raises(Exception) as ex:
            qb.improve(s.ADMM, num_iters=5, rho=rho_small, setup=setup_)
        assert qb.last_stats is None and qb.engine.last_admm_kernel()[0] == ''      # before any ADMM launch
        text[setup_] = str(ex.value)
        f, v = qb.improve(s.ADMM, num_iters=5, rho=rho_ok, setup=setup_)
        assert np.array_equal(qb.last_stats['rho'], np.full(3, rho_ok))
        qb.close()
    assert text['device'] == text['host'] and text['host'].startswith('rho parameter is too small')


def test_refusals_leave_the_context_alone(eng_mod):
    from qcqp_amd import problems

    def refused(funcs, code, word, B=2, P0s=None, raw=None, **kw):
        e = make(eng_mod, funcs)
        e.randn(19, seed=3)
        before, (f0, mv), kern, akern = e.download(), e.eval(), e.last_cd_kernel(), e.last_admm_kernel()
        n = e.n
        if raw is not None:                   # what the method itself would not pass on
            rc, msg = raw(e), e.L.qcqpmi_last_error(e.h).decode()
            assert rc == code and word in msg, (rc, msg)
        else:
            with pytest.raises(eng_mod.EngineError) as ex:
                e.admm_batch_setup(np.zeros((B, n, n)) if P0s is None else P0s, **kw)
            assert ex.value.code == code and word in str(ex.value), (ex.value.code, str(ex.value))
        assert e.pop_size == 19 and np.array_equal(e.download(), before)
        assert e.last_cd_kernel() == kern and e.last_admm_kernel() == akern
        f1, mv1 = e.eval()
        assert np.array_equal(f0, f1) and np.array_equal(mv, mv1)
        e.close()

    refused(problems.boolean_least_squares(129, 140, seed=1)[0], -4, 'n = 129')
    funcs = problems.boolean_least_squares(70, 80, seed=1)[0]
    P = np.zeros((70, 70))
    P[3, 68] = P[68, 3] = 0.5
    refused(funcs + [(P, np.zeros(70), -1.0, '<=')], -4, 'not separable')
    refused(funcs, -1, 'B = 0', B=0)
    refused(funcs, -1, 'P0s are missing',
            raw=lambda e: e.L.qcqpmi_admm_batch_setup(e.h, 2, None, None, 30, 1e-15, None, None, None, None, None))
    refused(funcs, -1, 'max_sweeps = 0', max_sweeps=0)
    for tol in (0.0, -1e-15, np.inf, np.nan):
        refused(funcs, -1, 'tol', tol=tol)
    for rho in (0.0, -1.0, np.inf, np.nan):
        refused(funcs, -1, 'rho', rho=rho)
    refused(funcs[:1], -1, 'no constraint')
    for n in (33, 128):                        # found while staging: the call fails after its launch and returns no results
        big = problems.boolean_least_squares(n, n + 2, seed=1)[0]
        asym = np.zeros((2, n, n))
        asym[1, n // 2 + 3, n - 1] = 1.0
        refused(big, -1, 'not symmetric', P0s=asym)
        nan = np.zeros((2, n, n))
        nan[0, n - 1, n - 1] = np.nan
        refused(big, -1, 'not symmetric', P0s=nan)

    # around a successful call: the population, its evaluation and the two kernel names stay
    fl = ab.family('bls', 33, 2, seed=4)
    e = make(eng_mod, fl[0])
    e.randn(19, seed=3)
    e.cd_run(seed=3)
    before = (e.download(), e.last_cd_kernel(), e.last_admm_kernel(), e.eval())
    assert before[1]
    o = e.admm_batch_setup(ab.objectives(fl)[0])
    assert (o['status'] == 0).all()
    after = (e.download(), e.last_cd_kernel(), e.last_admm_kernel(), e.eval())
    assert e.pop_size == 19 and np.array_equal(before[0], after[0]) and before[1:3] == after[1:3]
    assert np.array_equal(before[3][0], after[3][0]) and np.array_equal(before[3][1], after[3][1])
    # any output may be NULL
    assert e.L.qcqpmi_admm_batch_setup(e.h, 2, eng_mod._dp(ab.objectives(fl)[0]), None, 30, 1e-15, None, None, None, None, None) == 0
    e.close()
