"""qcqpmi_sdr_small_batch (sdr_small_kernel, csrc/sdr_small.hip): suggest(SDR) for B small problems (n <= 64) with shared constraints
x_i^2 == d_i in one launch -- the relaxation by the mixing method, its multipliers and S samples per problem.  The reference hands the
relaxation to a third-party solver, so there is no parity target: EVERY problem of the grid (tests/sdr_batch_cases.py: n in {1, 2, 7,
31, 32, 33, 63, 64} x Boolean least squares / weighted MAXCUT / rescaled x_i^2 == d_i, the nine (B, S) pairs of {1, 3, 64} x {1, 17,
64} dealt round-robin, tol = 1e-13, max_sweeps = 20000) is checked by its optimality conditions -- unit rows 1e-12, primal against
<C, V V^T> 1e-9, y against sdr.dual_certificate 1e-9 (1 + max |C|), sweeps under the limit and lambda_min >= -1e-6 (1 + max |C|) (the
project's own threshold; tests/test_sdr_batch_cpu.py shows a tenfold margin on this grid), bound <= primal, bound <= brute force for
n <= 7 -- and EVERY coordinate of EVERY sample against x = s o (V_n u + V_n (xi - u (u . xi))) rebuilt on the host from the returned V
and the oracle's keyed normals, 1e-12 (1 + max |x|).  Also: the existing single-problem solver from the same start, bit-for-bit
invariance under the batch size, the order of the problems and a split of the samples, a batch larger than the device holds at
once (the waves draw further tickets), the documented keyed start, S = 0, the five
refusals, the QCQPBatch facade.  Without the feature every test fails (the symbol does not exist).

"bound <= primal" and "bound <= brute force" hold in exact arithmetic for ANY y; in doubles the three numbers carry the rounding of
their own evaluation, so the comparisons allow ROUND(C, y) = N^2 eps (max |y| + N max |C|): N eps |S|_2 is the backward error of
eigvalsh on S = C + diag(y), |S|_2 <= max |y| + N max |C|, and the bound multiplies lambda_min by N; the N-term sums -sum(y), <C, V V^T>
and x' P0 x stay below the same figure.  For N = 65 that is 1e-12 (max |y| + 65 max |C|).
Run with `-m gpu` on an MI355X.  Running time of the file there: 21 s (34 tests; the slowest, the documented start, 7.5 s of host-side keyed normals)."""

import numpy as np
import pytest

import sdr_batch_cases as sc
from life_oracle import check_restart, make, oracle_runs

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KEYS = ('V', 'y', 'primal', 'sweeps', 'X')


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def run(eng_mod, fl, S, seed=5, stride=1, fi=0, engine=None, max_sweeps=sc.MAX_SWEEPS, tol=sc.TOL, **kw):
    e = engine or make(eng_mod, fl[0])
    P0s, q0s, r0s = sc.objectives(fl)
    o = e.sdr_small_batch(P0s, q0s, r0s, S, max_sweeps=max_sweeps, tol=tol, seed=seed, seed_stride=stride, first_index=fi, **kw)
    if engine is None:
        e.close()
    return o


def rounding(C, y):
    N = C.shape[0]
    return N * N * EPS * (np.max(np.abs(y)) + N * np.max(np.abs(C)))


def check_relaxation(fl, o, tag):
    """The optimality conditions of every problem; returns (C, certificate of the batch)."""
    from qcqp_amd import sdr
    P0s, q0s, r0s = sc.objectives(fl)
    d = sc.d_of(fl[0])
    C = sc.lifted(P0s, q0s, r0s, d)
    cert = sdr.certify_batch(C, o['y'], o['sweeps'], sc.MAX_SWEEPS)
    for b in range(len(fl)):                  # every problem: none is left out
        t = tag + (b,)
        V, y, primal, scale = o['V'][b], o['y'][b], o['primal'][b], 1.0 + np.max(np.abs(C[b]))
        assert np.max(np.abs(np.einsum('ik,ik->i', V, V) - 1.0)) <= 1e-12, t
        host = float(np.einsum('ij,ik,jk->', C[b], V, V))
        assert abs(primal - host) <= 1e-9 * (1.0 + abs(host)), (t, primal, host)
        y_ref, lmin_ref, _ = sdr.dual_certificate(C[b], V)
        assert np.max(np.abs(y - y_ref)) <= 1e-9 * scale, (t, np.max(np.abs(y - y_ref)))
        lmin, bound = cert['lambda_min'][b], cert['bound'][b]
        print('%s sweeps %d lambda_min / scale %.3e gap %.3e' % (t, o['sweeps'][b], lmin / scale, primal - bound))
        assert abs(lmin - lmin_ref) <= 1e-9 * scale and cert['scale'][b] == scale, t
        assert 0 < o['sweeps'][b] < sc.MAX_SWEEPS, (t, o['sweeps'][b])
        assert lmin >= -1e-6 * scale and cert['converged'][b], (t, lmin, scale)
        assert bound <= primal + rounding(C[b], y), (t, bound, primal)
        if d.size <= 7:
            best = sc.brute_force(P0s[b], q0s[b], r0s[b], d)
            assert bound <= best + rounding(C[b], y), (t, bound, best)
    return C, cert


def host_samples(orc, V, s, S, seed_b, fi):
    """x (S, n) = s o (V_n u + V_n (xi - u (u . xi))), xi_k = the keyed normal (seed_b, fi + sample, k)."""
    n = s.size
    Vn, u = V[:n], V[n]
    mu = Vn.dot(u)
    X = np.empty((S, n))
    for sg in range(S):
        xi = np.array([orc.keyed_normal(seed_b, fi + sg, k) for k in range(sc.K)])
        X[sg] = s * (mu + Vn.dot(xi - u * u.dot(xi)))
    return X


def check_samples(orc, fl, o, S, seed, stride, fi, tag):
    s = np.sqrt(sc.d_of(fl[0]))
    assert o['X'].shape == (len(fl), S, s.size)
    for b in range(len(fl)):
        ref = host_samples(orc, o['V'][b], s, S, seed + b * stride, fi)
        err = np.max(np.abs(o['X'][b] - ref))
        assert err <= 1e-12 * (1.0 + np.max(np.abs(ref))), (tag, b, err)


@pytest.mark.parametrize('case', sc.cases(), ids=lambda c: '%s-n%d-B%d-S%d' % c[:4])
def test_every_problem_and_every_sample_of_the_grid(eng_mod, orc, case):
    name, n, B, S, pseed, seed, stride, fi = case
    fl = sc.family(name, n, B, seed=pseed)
    o = run(eng_mod, fl, S, seed=seed, stride=stride, fi=fi)
    check_relaxation(fl, o, (name, n, B, S))
    check_samples(orc, fl, o, S, seed, stride, fi, (name, n, B, S))
    if name == 'cut':       # q0 = 0: the homogenising row's g is zero on every sweep and the row stays where it started
        V0 = sc.keyed_starts(orc, B, n + 1, seed, stride)
        assert np.max(np.abs(o['V'][:, n, :] - V0[:, n, :])) <= 1e-13


@pytest.mark.parametrize('name,n', [('bls', 7), ('cut', 33), ('scaled', 64)])
def test_against_the_single_problem_solver_from_the_same_start(eng_mod, name, n):
    """qcqpmi_sdr_solve_unitdiag (component-sliced, one problem per cooperative launch) and the batch from ONE start: both certify,
    both rigorous bounds lie at or below both primal values, and the primal values differ by no more than the larger of the two
    certified gaps of the problem."""
    from qcqp_amd import sdr
    B = 3
    fl = sc.family(name, n, B, seed=21)
    rs = np.random.RandomState(n)
    V0 = rs.randn(B, n + 1, sc.K)
    V0 /= np.linalg.norm(V0, axis=2)[:, :, None]
    e = make(eng_mod, fl[0])
    o = run(eng_mod, fl, 0, engine=e, V0s=V0)
    C, cert = check_relaxation(fl, o, ('single', name, n))
    for b in range(B):
        V1, hist, sw = e.sdr_solve_unitdiag(C[b], V0=V0[b], max_sweeps=sc.MAX_SWEEPS, tol=sc.TOL)
        y1, lmin1, bound1 = sdr.dual_certificate(C[b], V1)
        scale = 1.0 + np.max(np.abs(C[b]))
        assert sw < sc.MAX_SWEEPS and lmin1 >= -1e-6 * scale, (name, n, b, sw, lmin1)
        p1, p2, bound2 = float(hist[-1]), o['primal'][b], cert['bound'][b]
        rnd = max(rounding(C[b], y1), rounding(C[b], o['y'][b]))
        print('%s n %d b %d: primal %.15g / %.15g, gaps %.3e / %.3e' % (name, n, b, p1, p2, p1 - bound1, p2 - bound2))
        assert max(bound1, bound2) <= min(p1, p2) + rnd, (name, n, b, bound1, bound2, p1, p2)
        assert abs(p1 - p2) <= max(p1 - bound1, p2 - bound2) + rnd, (name, n, b, p1, p2, bound1, bound2)
    e.close()


def same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def test_invariance_bit_for_bit(eng_mod, orc):
    n, S = 31, 64
    fl = sc.family('scaled', n, 64, seed=4)
    e = make(eng_mod, fl[0])
    o = run(eng_mod, fl, S, seed=4, stride=2, engine=e)
    for b in range(64):                       # a batch of 64 = 64 batches of 1
        o1 = run(eng_mod, [fl[b]], S, seed=4 + 2 * b, stride=2, engine=e)
        for k in KEYS:
            assert np.array_equal(o[k][b], o1[k][0]), (b, k)
    perm = np.random.RandomState(0).permutation(64)     # the order of the problems (one seed for all: stride 0)
    oa = run(eng_mod, fl, S, seed=4, stride=0, engine=e)
    ob = run(eng_mod, [fl[p] for p in perm], S, seed=4, stride=0, engine=e)
    for k in KEYS:
        assert np.array_equal(oa[k][perm], ob[k]), k
    h0 = run(eng_mod, fl, 32, seed=4, stride=2, fi=0, engine=e)     # S = 64 at first_index 0 = S = 32 at 0 and at 32; V equal in all
    h1 = run(eng_mod, fl, 32, seed=4, stride=2, fi=32, engine=e)
    same(o, h0, KEYS[:4])
    same(o, h1, KEYS[:4])
    assert np.array_equal(o['X'], np.concatenate([h0['X'], h1['X']], axis=1))
    e.close()


def test_more_problems_than_resident_waves(eng_mod):
    """B = 16384 problems of n = 2: more than the device holds at once (at most 32 one-wave workgroups per CU), so the waves draw
    further tickets and reuse their LDS image.  Problems spread over the batch equal batches of one, bit for bit."""
    B, S = 16384, 1
    base = sc.family('scaled', 2, 8, seed=6)
    fl = [base[b % 8] for b in range(B)]
    e = make(eng_mod, fl[0])
    o = run(eng_mod, fl, S, seed=9, stride=1, fi=2, engine=e)
    assert (o['sweeps'] > 0).all() and (o['sweeps'] < sc.MAX_SWEEPS).all()
    for b in (0, 1, 255, 256, 4097, 8191, 12345, B - 2, B - 1):
        o1 = run(eng_mod, [fl[b]], S, seed=9 + b, stride=1, fi=2, engine=e)
        for k in KEYS:
            assert np.array_equal(o[k][b], o1[k][0]), (b, k)
    e.close()


def test_the_documented_start(eng_mod, orc):
    """max_sweeps = 0 returns the start.  The device's keyed start IS the documented one (csrc/sdr_small.h) rebuilt on the host -- to
    1e-13, the slack every test of the keyed normals gives the device's log / sin / cos against glibc's, not bit for bit --, its rows
    are unit, and a start handed back through V0s is taken as it is: the same results, bit for bit."""
    for n, B in ((7, 3), (64, 3)):
        fl = sc.family('bls', n, B, seed=9)
        e = make(eng_mod, fl[0])
        start = run(eng_mod, fl, 0, seed=13, stride=5, engine=e, max_sweeps=0)
        assert (start['sweeps'] == 0).all()
        host = sc.keyed_starts(orc, B, n + 1, 13, 5)
        assert np.max(np.abs(start['V'] - host)) <= 1e-13, n
        assert np.max(np.abs(np.einsum('bik,bik->bi', start['V'], start['V']) - 1.0)) <= 1e-12
        a = run(eng_mod, fl, 17, seed=13, stride=5, fi=3, engine=e)
        b = run(eng_mod, fl, 17, seed=13, stride=5, fi=3, engine=e, V0s=start['V'])
        same(a, b)
        c = run(eng_mod, fl, 17, seed=13, stride=5, fi=3, engine=e, V0s=host)       # the host's rebuild: a certified solve as well
        check_relaxation(fl, c, ('host start', n))
        check_samples(orc, fl, c, 17, 13, 5, 3, ('host start', n))
        e.close()


def test_no_samples(eng_mod):
    """S = 0: the relaxation alone (X is NULL in the call); the same V, y, primal and sweeps as with samples."""
    fl = sc.family('bls', 33, 3, seed=6)
    e = make(eng_mod, fl[0])
    o0 = run(eng_mod, fl, 0, seed=8, engine=e)
    assert o0['X'].shape == (3, 0, 33)
    check_relaxation(fl, o0, ('S = 0',))
    same(o0, run(eng_mod, fl, 17, seed=8, engine=e), KEYS[:4])
    P0s, q0s, r0s = sc.objectives(fl)      # every output NULL: the call still runs
    from qcqp_amd.engine import _dp
    assert e.L.qcqpmi_sdr_small_batch(e.h, 3, _dp(P0s), _dp(q0s), _dp(r0s), 0, 50, 1e-9, 8, 1, 0, None, None, None, None, None, None) == 0
    e.close()


def test_refusals_leave_the_population_alone(eng_mod):
    from qcqp_amd import problems

    def refused(funcs, B, code, P0s=None):
        e = make(eng_mod, funcs)
        e.randn(19, seed=3)
        before = e.download()
        f0, mv = e.eval()
        kernel = e.last_cd_kernel()
        n = e.n
        with pytest.raises(eng_mod.EngineError) as ex:
            e.sdr_small_batch(np.zeros((B, n, n)) if P0s is None else P0s, np.zeros((B, n)), np.zeros(B), 4)
        assert ex.value.code == code, (ex.value.code, str(ex.value))
        assert e.pop_size == 19 and np.array_equal(e.download(), before) and e.last_cd_kernel() == kernel
        f1, mv1 = e.eval()
        assert np.array_equal(f0, f1) and np.array_equal(mv, mv1)
        e.close()

    refused(problems.box_qp(16, seed=1, lo=-1.0, hi=1.0)[0], 2, -4)              # a box-constrained problem
    refused(problems.boolean_least_squares(65, 70, seed=1)[0], 2, -4)            # n = 65
    funcs = problems.boolean_least_squares(16, 20, seed=1)[0]
    P = np.zeros((16, 16))
    P[0, 1] = P[1, 0] = 0.5
    refused(funcs + [(P, np.zeros(16), -1.0, '<=')], 2, -4)                      # a coupled constraint
    refused(funcs, 0, -1)                                                        # B = 0
    P0s = np.zeros((2, 16, 16))                                                  # a P0_b that is not symmetric
    P0s[1, 2, 3] = 1.0
    refused(funcs, 2, -1, P0s=P0s)


def test_a_successful_call_leaves_the_population_alone(eng_mod):
    """The resident population, its evaluation, its status codes and the kernel name of the last run stay as they were."""
    import ctypes as C

    def status(e):
        st1, st2 = np.zeros(19, dtype=np.int32), np.zeros(19, dtype=np.int32)
        assert e.L.qcqpmi_cd_status(e.h, st1.ctypes.data_as(C.POINTER(C.c_int)), st2.ctypes.data_as(C.POINTER(C.c_int))) == 0
        return st1, st2

    fl = sc.family('bls', 16, 3, seed=2)
    e = make(eng_mod, fl[0])
    e.randn(19, seed=3)
    e.cd_run(seed=3)
    X, (f, mv), st, kernel = e.download(), e.eval(), status(e), e.last_cd_kernel()
    run(eng_mod, fl, 5, engine=e)
    assert e.pop_size == 19 and np.array_equal(e.download(), X) and e.last_cd_kernel() == kernel and kernel
    f1, mv1 = e.eval()
    assert np.array_equal(f, f1) and np.array_equal(mv, mv1)
    assert np.array_equal(st[0], status(e)[0]) and np.array_equal(st[1], status(e)[1])
    e.close()


def test_facade(eng_mod, orc):
    from qcqp_amd import problems, settings as s
    from qcqp_amd.batch import QCQPBatch
    B, n, R, seed = 4, 24, 32, 17
    fl = problems.boolean_least_squares_batch(B, n, 36, seed=2)
    qb = QCQPBatch(fl)
    qb.suggest(s.SDR, num_samples=R, seed=seed)
    assert qb.sdr_bound.shape == (B,) and qb.sdr_info['converged'].all() and np.isfinite(qb.sdr_bound).all()
    assert set(('primal', 'sweeps', 'lambda_min', 'converged')) <= set(qb.sdr_info)
    X0 = qb._starts.copy()
    assert X0.shape == (B, R, n)
    f, v = qb.improve(s.COORD_DESCENT, num_iters=200)
    assert (qb.sdr_bound <= f).all(), (qb.sdr_bound, f)
    assert qb.last_stats['kernel'] == 'cd_small_kernel<1>'
    # the same launch called directly on the samples: bit for bit
    e = make(eng_mod, fl[0])
    P0s, q0s, r0s = sc.objectives(fl)
    o = e.cd_small_batch_run(P0s, q0s, r0s, R, X0=X0, num_iters=200, seed=seed)
    e.close()
    assert np.array_equal(qb.population_f, o['f0']) and np.array_equal(qb.population_v, o['maxviol']) and np.array_equal(qb.x, o['best_x'])
    assert np.array_equal(f, o['best_f0']) and np.array_equal(v, o['best_maxviol']) and np.array_equal(qb.best_index, o['best_index'])
    counters = ('sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2')
    for k in counters:
        assert np.array_equal(qb.last_stats[k], o[k]), k
    # every restart from the samples against the oracle's improve_cd_sep from the same start
    for b in range(B):
        prob = orc.Problem(fl[b])
        res = oracle_runs(orc, prob, [(X0[b, r], seed + b, r) for r in range(R)], 200)
        ob = dict((k, o[k][b]) for k in counters + ('f0', 'maxviol'))
        Xb = np.ascontiguousarray(o['X'][b].T)
        for r, rr in enumerate(res):
            check_restart(ob, Xb, r, rr, 200, ('facade', b))
    # suggest(RANDOM) + improve on the same object: what a fresh object gives (the code path of before: keyed normals in the launch)
    qb.suggest(s.RANDOM, num_samples=R, seed=seed, first_index=3)
    f2, v2 = qb.improve(s.COORD_DESCENT, num_iters=200)
    fresh = QCQPBatch(fl)
    fresh.suggest(s.RANDOM, num_samples=R, seed=seed, first_index=3)
    f3, v3 = fresh.improve(s.COORD_DESCENT, num_iters=200)
    assert qb.last_stats['kernel'] == 'cd_small_kernel<1>'
    assert np.array_equal(f2, f3) and np.array_equal(v2, v3) and np.array_equal(qb.x, fresh.x)
    assert np.array_equal(qb.population_f, fresh.population_f) and np.array_equal(qb.population_v, fresh.population_v)
    assert np.array_equal(qb.best_index, fresh.best_index)
    # SDR refuses what sdr.unit_diagonal_family refuses
    qbox = QCQPBatch(problems.box_qp_batch(8, [1, 2], lo=-1.0, hi=1.0))
    with pytest.raises(Exception):
        qbox.suggest(s.SDR, num_samples=4)
    for q in (qb, fresh, qbox):
        q.close()
