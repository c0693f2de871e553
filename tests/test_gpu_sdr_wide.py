"""qcqpmi_sdr_batch / qcqpmi_sdr_batch_pc (sdr_small_kernel<true>, csrc/sdr_small.hip): suggest(SDR) for B problems of 65 to 128
variables with constraints x_i^2 == d_i in one launch -- C_b packed in LDS, two coordinates per lane in the samples.  EVERY problem of
the grid (tests/sdr_wide_cases.py: n in {65, 66, 95, 96, 97, 127, 128} x Boolean least squares / weighted MAXCUT / rescaled
x_i^2 == d_i, the six (B, S) pairs of {1, 3} x {1, 17, 64} dealt round-robin, tol = 1e-13, max_sweeps = 20000) is checked by its
optimality conditions with the thresholds of tests/test_gpu_sdr_batch.py -- unit rows 1e-12, primal against <C, V V^T> 1e-9, y against
sdr.dual_certificate 1e-9 (1 + max |C|), 0 < sweeps < the limit, lambda_min >= -1e-6 (1 + max |C|) (tests/test_sdr_wide_cpu.py shows a
tenfold margin on this grid), bound <= primal -- and EVERY coordinate of EVERY sample against x = s o (V_n u + V_n (xi - u (u . xi)))
rebuilt on the host from the returned V and the oracle's keyed normals, 1e-12 (1 + max |x|).  n is past brute force, so in its place
the bound must not exceed the objective at the Boolean point s o sign(x) of every returned sample.  Also: V and primal sweep by sweep
against the exact-order restatement (1e-12), the single-problem solver from the same start, the old symbol against the new one at
n <= 64 (bit for bit), bit-for-bit invariance under the batch size, the order of the problems and a split of the samples, per-problem
d against the shared call on the problem's own context, more problems than the device holds waves, the documented keyed start, S = 0,
a coordinate of the second slot alone, the refusals, the QCQPBatch facade with wide=True.  Without the feature every test but the
old-and-new-symbol one fails at the missing symbol (that one fails too: it calls the new symbol).

The comparisons of a bound with a primal value or an objective allow ROUND(C, y) = N^2 eps (max |y| + N max |C|), as
tests/test_gpu_sdr_batch.py derives it.  No cap on the workgroup count is exposed by the engine, so that invariance is not tested.
Run with `-m gpu` on an MI355X.  Running time of the file there: 22 s (41 tests; the slowest, the grid's scaled n = 128 with a problem of
4306 sweeps, 3.5 s).  Measured sweep by sweep: V within 2.8e-16, primal 4.4e-16, y 1.5e-15 of the restatement."""

import numpy as np
import pytest

import sdr_batch_cases as sc
import sdr_wide_cases as wc
from life_oracle import make

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KEYS = ('V', 'y', 'primal', 'sweeps', 'X')


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def run(eng_mod, fl, S, seed=5, stride=1, fi=0, engine=None, max_sweeps=wc.MAX_SWEEPS, tol=wc.TOL, entry='sdr_batch', **kw):
    e = engine or make(eng_mod, fl[0])
    P0s, q0s, r0s = sc.objectives(fl)
    o = getattr(e, entry)(P0s, q0s, r0s, S, max_sweeps=max_sweeps, tol=tol, seed=seed, seed_stride=stride, first_index=fi, **kw)
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
    cert = sdr.certify_batch(C, o['y'], o['sweeps'], wc.MAX_SWEEPS)
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
        assert 0 < o['sweeps'][b] < wc.MAX_SWEEPS, (t, o['sweeps'][b])
        assert lmin >= -1e-6 * scale and cert['converged'][b], (t, lmin, scale)
        assert bound <= primal + rounding(C[b], y), (t, bound, primal)
        if o['X'].shape[1]:                   # in place of the brute force: the Boolean point of every sample is feasible
            s = np.sqrt(d)
            Xr = s * np.where(o['X'][b] >= 0.0, 1.0, -1.0)
            fx = np.einsum('si,ij,sj->s', Xr, P0s[b], Xr) + Xr.dot(q0s[b]) + r0s[b]
            assert bound <= fx.min() + rounding(C[b], y), (t, bound, fx.min())
    return C, cert


def host_samples(orc, V, s, S, seed_b, fi):
    """x (S, n) = s o (V_n u + V_n (xi - u (u . xi))), xi_k = the keyed normal (seed_b, fi + sample, k); n up to 128."""
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


@pytest.mark.parametrize('case', wc.cases(), ids=lambda c: '%s-n%d-B%d-S%d' % c[:4])
def test_every_problem_and_every_sample_of_the_grid(eng_mod, orc, case):
    name, n, B, S, pseed, seed, stride, fi = case
    fl = sc.family(name, n, B, seed=pseed)
    o = run(eng_mod, fl, S, seed=seed, stride=stride, fi=fi)
    check_relaxation(fl, o, (name, n, B, S))
    check_samples(orc, fl, o, S, seed, stride, fi, (name, n, B, S))
    if name == 'cut':       # q0 = 0: the homogenising row's g is zero on every sweep and the row stays where it started
        V0 = sc.keyed_starts(orc, B, n + 1, seed, stride)
        assert np.max(np.abs(o['V'][:, n, :] - V0[:, n, :])) <= 1e-13


@pytest.mark.parametrize('name,n', [('bls', 65), ('bls', 66), ('bls', 97), ('bls', 128), ('cut', 128)])
def test_sweep_by_sweep_against_the_exact_order_restatement(eng_mod, name, n):
    """V0s given, tol = 0, max_sweeps = 1 and 3: V, primal and y against the restatement that sums in the kernel's order (N mod 4 = 2,
    3, 2, 1: the remainder of the four partial sums), 1e-12 as tests/test_gpu_sdr_mixing.py."""
    fl = sc.family(name, n, 1, seed=5)
    P0s, q0s, r0s = sc.objectives(fl)
    C = sc.lifted(P0s, q0s, r0s, sc.d_of(fl[0]))[0]
    rs = np.random.RandomState(n)
    V0 = rs.randn(1, n + 1, sc.K)
    V0 /= np.linalg.norm(V0, axis=2)[:, :, None]
    e = make(eng_mod, fl[0])
    for k in (1, 3):
        o = run(eng_mod, fl, 0, engine=e, max_sweeps=k, tol=0.0, V0s=V0)
        V, f, primal, y = wc.exact_sweeps(C, V0[0], k)
        errs = (np.max(np.abs(o['V'][0] - V)), abs(o['primal'][0] - primal) / (1.0 + abs(primal)),
                np.max(np.abs(o['y'][0] - y)) / (1.0 + np.max(np.abs(y))))
        print('%s n %d sweeps %d: V %.3e primal %.3e y %.3e' % ((name, n, k) + errs))
        assert o['sweeps'][0] == k
        assert errs[0] <= 1e-12 and errs[1] <= 1e-12 and errs[2] <= 1e-12, (name, n, k, errs)
        assert abs(f - primal) <= 1e-12 * (1.0 + abs(primal))      # the tracked objective is the recomputed one
    e.close()


@pytest.mark.parametrize('name,n', [('bls', 65), ('cut', 97), ('scaled', 128)])
def test_against_the_single_problem_solver_from_the_same_start(eng_mod, name, n):
    """qcqpmi_sdr_solve_unitdiag (component-sliced, one problem per cooperative launch) and the batch from ONE start: both certify,
    both rigorous bounds lie at or below both primal values, and the primal values differ by no more than the larger of the two
    certified gaps of the problem (the assertions of tests/test_gpu_sdr_batch.py)."""
    from qcqp_amd import sdr
    B = 1
    fl = sc.family(name, n, B, seed=21)
    rs = np.random.RandomState(n)
    V0 = rs.randn(B, n + 1, sc.K)
    V0 /= np.linalg.norm(V0, axis=2)[:, :, None]
    e = make(eng_mod, fl[0])
    o = run(eng_mod, fl, 0, engine=e, V0s=V0)
    C, cert = check_relaxation(fl, o, ('single', name, n))
    for b in range(B):
        V1, hist, sw = e.sdr_solve_unitdiag(C[b], V0=V0[b], max_sweeps=wc.MAX_SWEEPS, tol=wc.TOL)
        y1, lmin1, bound1 = sdr.dual_certificate(C[b], V1)
        scale = 1.0 + np.max(np.abs(C[b]))
        assert sw < wc.MAX_SWEEPS and lmin1 >= -1e-6 * scale, (name, n, b, sw, lmin1)
        p1, p2, bound2 = float(hist[-1]), o['primal'][b], cert['bound'][b]
        rnd = max(rounding(C[b], y1), rounding(C[b], o['y'][b]))
        print('%s n %d b %d: primal %.15g / %.15g, gaps %.3e / %.3e' % (name, n, b, p1, p2, p1 - bound1, p2 - bound2))
        assert max(bound1, bound2) <= min(p1, p2) + rnd, (name, n, b, bound1, bound2, p1, p2)
        assert abs(p1 - p2) <= max(p1 - bound1, p2 - bound2) + rnd, (name, n, b, p1, p2, bound1, bound2)
    e.close()


def same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize('n', [33, 64])
def test_old_and_new_symbol_are_bit_identical_up_to_64(eng_mod, n):
    B, S = 3, 17
    fl = sc.family('scaled', n, B, seed=4)
    e = make(eng_mod, fl[0])
    kw = dict(seed=4, stride=2, fi=3, engine=e, max_sweeps=300, tol=1e-11)
    same(run(eng_mod, fl, S, entry='sdr_small_batch', **kw), run(eng_mod, fl, S, entry='sdr_batch', **kw))
    ds = np.random.RandomState(n).uniform(0.25, 4.0, size=(B, n))
    a, b = run(eng_mod, fl, S, entry='sdr_small_batch', ds=ds, **kw), run(eng_mod, fl, S, entry='sdr_batch', ds=ds, **kw)
    same(a, b)
    assert (a['sweeps'] > 0).all() and np.isfinite(a['X']).all()
    e.close()


def test_invariance_bit_for_bit(eng_mod):
    n, S, B = 97, 64, 24
    fl = sc.family('scaled', n, B, seed=4)
    e = make(eng_mod, fl[0])
    kw = dict(engine=e, max_sweeps=40, tol=0.0)
    o = run(eng_mod, fl, S, seed=4, stride=2, **kw)
    assert (o['sweeps'] == 40).all()
    for b in range(B):                        # a batch of 24 = 24 batches of 1
        o1 = run(eng_mod, [fl[b]], S, seed=4 + 2 * b, stride=2, **kw)
        for k in KEYS:
            assert np.array_equal(o[k][b], o1[k][0]), (b, k)
    perm = np.random.RandomState(0).permutation(B)      # the order of the problems (one seed for all: stride 0)
    oa = run(eng_mod, fl, S, seed=4, stride=0, **kw)
    ob = run(eng_mod, [fl[p] for p in perm], S, seed=4, stride=0, **kw)
    for k in KEYS:
        assert np.array_equal(oa[k][perm], ob[k]), k
    h0 = run(eng_mod, fl, 32, seed=4, stride=2, fi=0, **kw)     # S = 64 at first_index 0 = S = 32 at 0 and at 32; V equal in all
    h1 = run(eng_mod, fl, 32, seed=4, stride=2, fi=32, **kw)
    same(o, h0, KEYS[:4])
    same(o, h1, KEYS[:4])
    assert np.array_equal(o['X'], np.concatenate([h0['X'], h1['X']], axis=1))
    e.close()


@pytest.mark.parametrize('n', [65, 96, 128])
def test_per_problem_d_equals_the_shared_call_on_the_problems_own_context(eng_mod, n):
    from qcqp_amd import problems
    B, S, seed, stride, fi = 3, 5, 21, 5, 7
    fl = problems.per_problem_constraints_batch('eqpp', n, [31, 32, 33])
    ds = np.stack([sc.d_of(f) for f in fl])
    assert not np.array_equal(ds[0], ds[-1])
    e = make(eng_mod, fl[0])
    o = run(eng_mod, fl, S, seed=seed, stride=stride, fi=fi, engine=e, max_sweeps=100, tol=0.0, ds=ds)
    e.close()
    assert o['X'].shape == (B, S, n) and (o['sweeps'] == 100).all()
    for b in range(B):
        o1 = run(eng_mod, [fl[b]], S, seed=seed + b * stride, stride=stride, fi=fi, max_sweeps=100, tol=0.0)
        for k in KEYS:
            assert np.array_equal(o[k][b], o1[k][0]), (n, b, k)


def test_more_problems_than_resident_waves(eng_mod):
    """B = 300 problems of n = 128: one workgroup per CU, so the waves draw further tickets and reuse their LDS image.  Problems at
    both ends and in the middle equal batches of one, bit for bit."""
    B, S = 300, 2
    base = sc.family('bls', 128, 6, seed=6)
    fl = [base[b % 6] for b in range(B)]
    e = make(eng_mod, fl[0])
    kw = dict(engine=e, max_sweeps=3, tol=0.0)
    o = run(eng_mod, fl, S, seed=9, stride=1, fi=2, **kw)
    assert (o['sweeps'] == 3).all() and np.isfinite(o['X']).all() and np.isfinite(o['V']).all()
    for b in (0, 150, 299):
        o1 = run(eng_mod, [fl[b]], S, seed=9 + b, stride=1, fi=2, **kw)
        for k in KEYS:
            assert np.array_equal(o[k][b], o1[k][0]), (b, k)
    e.close()


def test_the_documented_start(eng_mod, orc):
    """max_sweeps = 0 returns the start: the documented one (csrc/sdr_small.h) rebuilt on the host, 1e-15."""
    n, B = 100, 1
    fl = sc.family('bls', n, B, seed=9)
    start = run(eng_mod, fl, 0, seed=13, stride=5, max_sweeps=0)
    assert (start['sweeps'] == 0).all()
    host = sc.keyed_starts(orc, B, n + 1, 13, 5)
    assert np.max(np.abs(start['V'] - host)) <= 1e-15, np.max(np.abs(start['V'] - host))


def test_no_samples(eng_mod):
    """S = 0: the relaxation alone (X is NULL in the call, nothing is written); the same V, y, primal and sweeps as with samples."""
    from qcqp_amd.engine import _dp
    fl = sc.family('bls', 66, 2, seed=6)
    e = make(eng_mod, fl[0])
    kw = dict(seed=8, engine=e, max_sweeps=50, tol=0.0)
    o0 = run(eng_mod, fl, 0, **kw)
    assert o0['X'].shape == (2, 0, 66)
    same(o0, run(eng_mod, fl, 17, **kw), KEYS[:4])
    P0s, q0s, r0s = sc.objectives(fl)      # every output NULL: the call still runs
    assert e.L.qcqpmi_sdr_batch(e.h, 2, _dp(P0s), _dp(q0s), _dp(r0s), 0, 50, 1e-9, 8, 1, 0, None, None, None, None, None, None) == 0
    e.close()


def test_the_second_slot_alone_at_n_65(eng_mod, orc):
    """n = 65: coordinate 64 is the only one in slot 1 (lane 0).  x_64 against the host rebuild, by name."""
    n, S, seed, fi = 65, 9, 31, 4
    fl = sc.family('scaled', n, 1, seed=12)
    o = run(eng_mod, fl, S, seed=seed, fi=fi, max_sweeps=60, tol=0.0)
    s = np.sqrt(sc.d_of(fl[0]))
    ref = host_samples(orc, o['V'][0], s, S, seed, fi)
    x64, r64 = o['X'][0][:, 64], ref[:, 64]
    assert np.all(x64 != 0.0) and np.max(np.abs(x64 - r64)) <= 1e-12 * (1.0 + np.max(np.abs(ref))), (x64, r64)
    assert np.max(np.abs(o['X'][0] - ref)) <= 1e-12 * (1.0 + np.max(np.abs(ref)))


def test_refusals_leave_the_population_alone(eng_mod):
    from qcqp_amd import problems

    def refused(funcs, B, code, P0s=None, entry='sdr_batch', **kw):
        e = make(eng_mod, funcs)
        e.randn(19, seed=3)
        before = e.download()
        f0, mv = e.eval()
        kernel = e.last_cd_kernel()
        n = e.n
        with pytest.raises(eng_mod.EngineError) as ex:
            getattr(e, entry)(np.zeros((B, n, n)) if P0s is None else P0s, np.zeros((B, n)), np.zeros(B), 4, **kw)
        assert ex.value.code == code, (ex.value.code, str(ex.value))
        assert e.pop_size == 19 and np.array_equal(e.download(), before) and e.last_cd_kernel() == kernel
        f1, mv1 = e.eval()
        assert np.array_equal(f0, f1) and np.array_equal(mv, mv1)
        e.close()

    refused(problems.boolean_least_squares(129, 135, seed=1)[0], 2, -4)          # n = 129
    refused(problems.box_qp(80, seed=1, lo=-1.0, hi=1.0)[0], 2, -4)              # a box-constrained problem
    funcs = problems.boolean_least_squares(104, 110, seed=1)[0]
    P = np.zeros((104, 104))
    P[0, 1] = P[1, 0] = 0.5
    refused(funcs + [(P, np.zeros(104), -1.0, '<=')], 2, -4)                     # a coupled constraint
    for i, j in ((70, 100), (100, 70)):                                          # a P0_b that is not symmetric, in either triangle
        P0s = np.zeros((2, 104, 104))
        P0s[1, i, j] = 1.0
        refused(funcs, 2, -1, P0s=P0s)
    ds = np.ones((2, 104))
    ds[1, 77] = 0.0
    refused(funcs, 2, -1, ds=ds)                                                 # a d that is not positive
    refused(problems.boolean_least_squares(65, 70, seed=1)[0], 2, -4, entry='sdr_small_batch')      # the old symbol at n = 65


def test_facade_wide(eng_mod):
    from qcqp_amd import problems, settings as s
    from qcqp_amd.batch import QCQPBatch
    B, n, R, seed = 3, 96, 8, 17
    fl = problems.boolean_least_squares_batch(B, n, 144, seed=2)
    qb = QCQPBatch(fl)
    with pytest.raises(Exception, match='n <= 64') as ex:      # the default refuses as before and names the keyword
        qb.suggest(s.SDR, num_samples=R, seed=seed)
    assert 'SDR' in str(ex.value) and 'wide=True' in str(ex.value) and qb.sdr_bound is None
    qb.suggest(s.SDR, num_samples=R, seed=seed, wide=True)
    assert qb.sdr_bound.shape == (B,) and set(('primal', 'sweeps', 'lambda_min', 'converged')) <= set(qb.sdr_info)
    X0 = qb._starts.copy()
    assert X0.shape == (B, R, n) and np.isfinite(X0).all()
    P0s, q0s, r0s = sc.objectives(fl)
    C = sc.lifted(P0s, q0s, r0s, sc.d_of(fl[0]))
    f, v = qb.improve(s.COORD_DESCENT, num_iters=200)
    assert qb.last_stats['kernel'] == 'cd_small_kernel<1,w2>'
    N = n + 1
    for b in range(B):
        if qb.sdr_info['converged'][b] and v[b] <= 1e-6:      # |y_i| <= N max |C|
            rnd = N * N * EPS * 2 * N * np.max(np.abs(C[b]))
            assert f[b] >= qb.sdr_bound[b] - rnd, (b, f[b], qb.sdr_bound[b])
    assert qb.sdr_info['converged'].any()
    # the samples ARE the starts of the launch: the same launch called directly on them, bit for bit
    e = make(eng_mod, fl[0])
    o = e.cd_batch_run(P0s, q0s, r0s, R, X0=X0, num_iters=200, seed=seed)
    od = e.sdr_batch(P0s, q0s, r0s, R, seed=seed, want_V=False)      # the facade's settings: max_sweeps = 5000, tol = 1e-11
    e.close()
    assert np.array_equal(qb.population_f, o['f0']) and np.array_equal(qb.x, o['best_x']) and np.array_equal(f, o['best_f0'])
    assert np.array_equal(od['X'], X0) and np.array_equal(od['primal'], qb.sdr_info['primal'])
    fa, va = qb.improve(s.ADMM, num_iters=50, wide=True)              # ADMM from the same samples
    assert 'w2' in qb.last_stats['kernel'] and np.isfinite(fa).all() and fa.shape == (B,)
    qb.close()
