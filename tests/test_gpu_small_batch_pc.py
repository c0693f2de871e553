"""qcqpmi_cd_small_batch_run_pc / qcqpmi_sdr_small_batch_pc (cd_small_kernel<MAXC, pc>, sdr_small_kernel with a per-problem s): B small
problems (n <= 64) whose constraints share their STRUCTURE and bring their own coefficients, in one launch.
  * EVERY restart of EVERY problem of the grid -- the six families of problems.per_problem_constraints_batch x n in {1, 2, 7, 16, 17,
    31, 32, 33, 48, 63, 64}, the nine (B, R) pairs of {1, 3, 64} x {1, 17, 64} dealt round-robin -- against the fast separable oracle
    run on problem b's own functions (pinned to the restatement on these families by tests/test_small_batch_pc_cpu.py), by
    life_oracle.check_restart: point 1e-9 relative, every counter equal, objective 1e-9, max violation 1e-12; the winner of every
    problem; the kernel name;
  * bit identity with the existing path: problem b of the _pc call equals, np.array_equal on every output array, the shared call with
    B = 1 on a context made from problem b's functions at seed + b stride; a _pc call whose cons repeats the context's coefficients
    equals the shared call;
  * bit-for-bit invariance under a sub-batch, a permutation of the problems, a split of R over two calls, and with uploaded starts;
  * the three refusals, the resident population left alone;
  * SDR on eqpp at n in {1, 7, 32, 33, 64} x B in {1, 3, 64}: V, y, primal, sweeps and X bit-identical to the shared call with B = 1 on
    problem b's own context, every problem by its optimality conditions and every sample rebuilt on the host (the checks of
    tests/test_gpu_sdr_batch.py with problem b's own d), and the refusal of a non-positive d;
  * the QCQPBatch facade.
Without the feature every test fails (the symbols, the keywords and the generator do not exist).  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

import sdr_batch_cases as sc
import small_batch_pc_cases as pc
from life_oracle import make
from test_gpu_small_batch import BR, COUNTERS, NS, check_vs_oracle, objectives
from test_gpu_sdr_batch import host_samples, rounding

pytestmark = pytest.mark.gpu

KEYS = COUNTERS + ('f0', 'maxviol', 'X', 'best_index', 'best_f0', 'best_maxviol', 'best_x')
SDR_KEYS = ('V', 'y', 'primal', 'sweeps', 'X')


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def run_pc(eng_mod, fl, R, seed=5, stride=1, fi=0, cons=None, **kw):
    """The _pc call on a context made from problem 0 (any problem of the list fixes the same structure)."""
    e = make(eng_mod, fl[0])
    P0s, q0s, r0s = objectives(fl)
    o = e.cd_small_batch_run(P0s, q0s, r0s, R, seed=seed, seed_stride=stride, first_index=fi, cons=pc.cons_of(fl) if cons is None else cons, **kw)
    o['kernel'] = e.last_cd_kernel()
    e.close()
    return o


def run_own(eng_mod, funcs, R, seed, fi=0, **kw):
    """The existing shared call with B = 1 on a context made from the problem's own functions."""
    e = make(eng_mod, funcs)
    P0s, q0s, r0s = objectives([funcs])
    o = e.cd_small_batch_run(P0s, q0s, r0s, R, seed=seed, seed_stride=1, first_index=fi, **kw)
    o['kernel'] = e.last_cd_kernel()
    e.close()
    return o


def pc_name(name):
    return 'cd_small_kernel<4,pc>' if name in pc.MAXC4 else 'cd_small_kernel<1,pc>'


@pytest.mark.parametrize('name', pc.FAMILIES)
def test_every_restart_of_every_problem_against_the_oracle(eng_mod, orc, name):
    k0 = pc.FAMILIES.index(name)
    for j, n in enumerate(NS):
        B, R = BR[(k0 + j) % len(BR)]
        fl = pc.family(name, n, B, seed=3 + j)
        o = run_pc(eng_mod, fl, R, seed=11 + j, stride=3, fi=5 * j)
        assert o['kernel'] == pc_name(name), (name, n, o['kernel'])
        check_vs_oracle(eng_mod, orc, fl, o, R, 11 + j, 3, 5 * j, (name, n, B, R))


@pytest.mark.parametrize('n', [7, 33, 64])
@pytest.mark.parametrize('name', ['boxpp', 'annpp', 'eqpp'])
def test_bit_identical_to_the_shared_call_on_the_problems_own_context(eng_mod, name, n):
    B, R, seed, stride, fi = 3, 17, 21, 5, 7
    fl = pc.family(name, n, B, seed=9)
    o = run_pc(eng_mod, fl, R, seed=seed, stride=stride, fi=fi)
    assert o['kernel'] == pc_name(name)
    for b in range(B):
        o1 = run_own(eng_mod, fl[b], R, seed + b * stride, fi)
        assert o1['kernel'] == ('cd_small_kernel<4>' if name in pc.MAXC4 else 'cd_small_kernel<1>')
        for k in KEYS:
            assert np.array_equal(o[k][b], o1[k][0]), (name, n, b, k)


@pytest.mark.parametrize('name,n', [('box11', 33), ('ann2', 17)])
def test_cons_that_repeats_the_contexts_coefficients_equals_the_shared_call(eng_mod, name, n):
    from test_gpu_small_batch import family
    B, R = 5, 17
    fl = family(name, n, B)
    e = make(eng_mod, fl[0])
    P0s, q0s, r0s = objectives(fl)
    a = e.cd_small_batch_run(P0s, q0s, r0s, R, seed=4, seed_stride=2, first_index=3)
    assert e.last_cd_kernel() == ('cd_small_kernel<4>' if name == 'ann2' else 'cd_small_kernel<1>')
    b = e.cd_small_batch_run(P0s, q0s, r0s, R, seed=4, seed_stride=2, first_index=3, cons=pc.cons_of(fl))
    assert e.last_cd_kernel() == ('cd_small_kernel<4,pc>' if name == 'ann2' else 'cd_small_kernel<1,pc>')
    e.close()
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


def test_invariance_bit_for_bit(eng_mod):
    fl = pc.family('boxpp', 31, 64)
    R = 64
    o = run_pc(eng_mod, fl, R, seed=4, stride=2)
    # a sub-batch: the seeds follow the problems (problems 5, 6, 7 at stride 2 from seed 4 + 2 * 5)
    for lst, sd in (([0], 4), ([63], 4 + 2 * 63), ([5, 6, 7], 4 + 2 * 5)):
        o1 = run_pc(eng_mod, [fl[b] for b in lst], R, seed=sd, stride=2)
        for k in KEYS:
            assert np.array_equal(o[k][lst], o1[k]), (lst, k)
    perm = np.random.RandomState(0).permutation(64)     # the order of the problems (one seed for all: stride 0)
    oa = run_pc(eng_mod, fl, R, seed=0, stride=0)
    ob = run_pc(eng_mod, [fl[p] for p in perm], R, seed=0, stride=0)
    for k in KEYS:
        assert np.array_equal(oa[k][perm], ob[k]), k
    for p in (0, 17, 63):                                # ... and a problem moved to another place with the seed it had in o
        o1 = run_pc(eng_mod, [fl[perm[p]]], R, seed=4 + 2 * int(perm[p]), stride=2)
        for k in KEYS:
            assert np.array_equal(o[k][perm[p]], o1[k][0]), (p, k)
    h0 = run_pc(eng_mod, fl, 32, seed=4, stride=2, fi=0)    # R = 64 at first_index 0 = R = 32 at 0 and at 32
    h1 = run_pc(eng_mod, fl, 32, seed=4, stride=2, fi=32)
    for k in COUNTERS + ('f0', 'maxviol', 'X'):
        assert np.array_equal(o[k], np.concatenate([h0[k], h1[k]], axis=1)), k


@pytest.mark.parametrize('name', ['eq2pp', 'annpp'])
def test_uploaded_starts(eng_mod, orc, name):
    n, B, R = 33, 3, 17
    fl = pc.family(name, n, B, seed=2)
    X0 = np.random.RandomState(5).randn(B, R, n)
    o = run_pc(eng_mod, fl, R, seed=8, X0=X0)
    for b in range(B):
        o1 = run_own(eng_mod, fl[b], R, 8 + b, X0=X0[b:b + 1])
        for k in KEYS:
            assert np.array_equal(o[k][b], o1[k][0]), (name, b, k)
    check_vs_oracle(eng_mod, orc, fl, o, R, 8, 1, 0, ('upload', name), X0=X0)


def test_refusals_leave_the_population_alone(eng_mod):
    from qcqp_amd.engine import _dp
    n, B, R = 16, 2, 4
    fl = pc.family('boxpp', n, B)
    P0s, q0s, r0s = objectives(fl)
    good = pc.cons_of(fl)
    e = make(eng_mod, fl[0])
    e.randn(19, seed=3)
    before = e.download()
    f0, mv = e.eval()

    def refused(call):
        with pytest.raises(eng_mod.EngineError) as ex:
            call()
        assert ex.value.code == -1, (ex.value.code, str(ex.value))
        assert e.pop_size == 19 and np.array_equal(e.download(), before)
        f1, mv1 = e.eval()
        assert np.array_equal(f0, f1) and np.array_equal(mv, mv1)

    def missing():                                       # cons == NULL in the call itself
        e._chk(e.L.qcqpmi_cd_small_batch_run_pc(e.h, B, _dp(P0s), _dp(q0s), _dp(r0s), None, R, 1, None, 1, 100, 1e-2, 1e-4, 1, 1, 0, 1e-4,
                                                None, None, None, None, None, None, None, None, None, None, None, None, None, None))
    refused(missing)
    for value in (np.nan, np.inf):
        bad = good.copy()
        bad[1, 5, 2] = value
        refused(lambda: e.cd_small_batch_run(P0s, q0s, r0s, R, cons=bad))
    bad = good.copy()
    bad[1, 3, :2] = 0.0                                  # p == 0 and q == 0: the constraint touches no coordinate
    refused(lambda: e.cd_small_batch_run(P0s, q0s, r0s, R, cons=bad))
    o = e.cd_small_batch_run(P0s, q0s, r0s, R, cons=good)       # and the call with the coefficients as they are succeeds
    assert (o['status1'] == 0).all() and e.pop_size == 19 and np.array_equal(e.download(), before)
    with pytest.raises(ValueError):
        e.cd_small_batch_run(P0s, q0s, r0s, R, cons=good[:, :-1])
    e.close()


# ---------------------------------------------------------------------------------------------------------------------- SDR
def run_sdr(e, fl, S, seed, stride, fi, ds=None):
    P0s, q0s, r0s = sc.objectives(fl)
    return e.sdr_small_batch(P0s, q0s, r0s, S, max_sweeps=sc.MAX_SWEEPS, tol=sc.TOL, seed=seed, seed_stride=stride, first_index=fi, ds=ds)


def check_relaxation(fl, ds, o, tag):
    """The optimality conditions of tests/test_gpu_sdr_batch.py's check_relaxation for every problem, with problem b's own d."""
    from qcqp_amd import sdr
    P0s, q0s, r0s = sc.objectives(fl)
    C = np.concatenate([sc.lifted(P0s[b:b + 1], q0s[b:b + 1], r0s[b:b + 1], ds[b]) for b in range(len(fl))])
    assert np.array_equal(C, sdr.lifted_cost_batch(P0s, q0s, r0s, ds))
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
        if ds.shape[1] <= 7:
            best = sc.brute_force(P0s[b], q0s[b], r0s[b], ds[b])
            assert bound <= best + rounding(C[b], y), (t, bound, best)


@pytest.mark.parametrize('case', pc.sdr_cases(), ids=lambda c: 'n%d-B%d' % c[:2])
def test_sdr_every_problem_every_sample_and_bit_identity(eng_mod, orc, case):
    from qcqp_amd import problems
    n, B, pseeds, seed, stride, fi = case
    S = 5
    fl = problems.per_problem_constraints_batch('eqpp', n, pseeds)
    ds = np.stack([sc.d_of(f) for f in fl])
    assert not np.array_equal(ds[0], ds[-1]) or B == 1
    e = make(eng_mod, fl[0])
    o = run_sdr(e, fl, S, seed, stride, fi, ds=ds)
    e.close()
    assert o['X'].shape == (B, S, n)
    for b in range(B):                        # bit for bit the shared call with B = 1 on problem b's own context
        eb = make(eng_mod, fl[b])
        o1 = run_sdr(eb, [fl[b]], S, seed + b * stride, stride, fi)
        eb.close()
        for k in SDR_KEYS:
            assert np.array_equal(o[k][b], o1[k][0]), (n, B, b, k)
    check_relaxation(fl, ds, o, ('eqpp', n, B))
    for b in range(B):                        # every sample of every problem rebuilt on the host
        ref = host_samples(orc, o['V'][b], np.sqrt(ds[b]), S, seed + b * stride, fi)
        err = np.max(np.abs(o['X'][b] - ref))
        assert err <= 1e-12 * (1.0 + np.max(np.abs(ref))), (n, B, b, err)


def test_sdr_refusals(eng_mod):
    from qcqp_amd import problems
    from qcqp_amd.engine import _dp
    n, B = 7, 3
    fl = pc.family('eqpp', n, B)
    ds = np.stack([sc.d_of(f) for f in fl])
    P0s, q0s, r0s = sc.objectives(fl)
    e = make(eng_mod, fl[0])
    e.randn(19, seed=3)
    before = e.download()
    for value in (0.0, -1.0, np.nan, np.inf):
        bad = ds.copy()
        bad[2, 4] = value
        with pytest.raises(eng_mod.EngineError) as ex:
            e.sdr_small_batch(P0s, q0s, r0s, 4, ds=bad)
        assert ex.value.code == -1, (value, ex.value.code)
        assert e.pop_size == 19 and np.array_equal(e.download(), before)
    assert e.L.qcqpmi_sdr_small_batch_pc(e.h, B, _dp(P0s), _dp(q0s), _dp(r0s), None, 0, 50, 1e-9, 8, 1, 0, None, None, None, None, None, None) == -1
    with pytest.raises(ValueError):
        e.sdr_small_batch(P0s, q0s, r0s, 4, ds=ds[:, :-1])
    e.close()
    box = pc.family('boxpp', n, B)            # a context outside the family: unsupported, as the shared call
    e = make(eng_mod, box[0])
    with pytest.raises(eng_mod.EngineError) as ex:
        e.sdr_small_batch(*objectives(box), 4, ds=ds)
    assert ex.value.code == -4
    e.close()


# ------------------------------------------------------------------------------------------------------------------- facade
def test_facade_random_and_improve_equals_the_engine_call(eng_mod):
    from qcqp_amd import settings as s
    from qcqp_amd.batch import QCQPBatch
    B, n, R, seed = 5, 24, 32, 17
    fl = pc.family('boxpp', n, B, seed=2)
    qb = QCQPBatch(fl)
    assert np.array_equal(qb.cons, pc.cons_of(fl))
    qb.suggest(s.RANDOM, num_samples=R, seed=seed, first_index=3, seed_stride=2)
    f, v = qb.improve(s.COORD_DESCENT, num_iters=200)
    assert qb.last_stats['kernel'] == 'cd_small_kernel<1,pc>' and qb.x.shape == (B, n)
    o = run_pc(eng_mod, fl, R, seed=seed, stride=2, fi=3, num_iters=200)
    assert np.array_equal(f, o['best_f0']) and np.array_equal(v, o['best_maxviol']) and np.array_equal(qb.x, o['best_x'])
    assert np.array_equal(qb.best_index, o['best_index'])
    assert np.array_equal(qb.population_f, o['f0']) and np.array_equal(qb.population_v, o['maxviol'])
    for k in COUNTERS:
        assert np.array_equal(qb.last_stats[k], o[k]), k
    assert (v < 1e-2).all()
    with pytest.raises(Exception):
        qb.suggest(s.SDR, num_samples=4)      # boxes are not of the unit-diagonal family
    qb.close()


def test_facade_sdr_and_improve_on_eqpp(eng_mod):
    from qcqp_amd import settings as s
    from qcqp_amd.batch import QCQPBatch
    B, n, R, seed = 4, 24, 32, 17
    fl = pc.family('eqpp', n, B, seed=2)
    ds = np.stack([sc.d_of(f) for f in fl])
    qb = QCQPBatch(fl)
    qb.suggest(s.SDR, num_samples=R, seed=seed)
    assert qb.sdr_bound.shape == (B,) and qb.sdr_info['converged'].all()
    X0 = qb._starts.copy()
    assert X0.shape == (B, R, n)
    f, v = qb.improve(s.COORD_DESCENT, num_iters=200)
    assert qb.last_stats['kernel'] == 'cd_small_kernel<1,pc>'
    cert = qb.sdr_info['converged']
    assert (qb.sdr_bound[cert] <= f[cert]).all(), (qb.sdr_bound, f)
    assert (v < 1e-2).all() and (np.abs(qb.x ** 2 - ds) < 1e-2).all()      # every winner satisfies its OWN constraints within viol_tol
    o2 = run_pc(eng_mod, fl, R, seed=seed, X0=X0, num_iters=200)
    assert np.array_equal(f, o2['best_f0']) and np.array_equal(qb.x, o2['best_x'])
    # the facade's suggest used max_sweeps = 5000, tol = 1e-11; the samples of a direct call with those settings are the facade's
    e = make(eng_mod, fl[0])
    P0s, q0s, r0s = sc.objectives(fl)
    od = e.sdr_small_batch(P0s, q0s, r0s, R, seed=seed, ds=ds, want_V=False)
    e.close()
    assert np.array_equal(od['X'], X0) and np.array_equal(od['primal'], qb.sdr_info['primal'])
    qb.close()


def test_facade_shared_constraints_keep_the_shared_kernel(eng_mod):
    from qcqp_amd import problems, settings as s
    from qcqp_amd.batch import QCQPBatch
    qb = QCQPBatch(problems.box_qp_batch(16, [1, 2, 3], lo=-1.0, hi=1.0))
    assert qb.cons is None
    qb.suggest(s.RANDOM, num_samples=8, seed=3)
    qb.improve(s.COORD_DESCENT, num_iters=100)
    assert qb.last_stats['kernel'] == 'cd_small_kernel<1>'
    qb.close()
