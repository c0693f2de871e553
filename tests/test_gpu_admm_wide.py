"""qcqpmi_admm_batch_run / QCQPBatch.improve(ADMM, wide=True): improve_admm (qcqp.py:254-285) for B problems of 65 <= n <= 128 variables
with separable constraints, R restarts each, in ONE launch of the wide kernels admm_small_kernel<MAXC[,pc],w2> (csrc/admm_small.hip;
DESIGN.md 4.14): one wavefront per (problem, restart), lane l holds the coordinates l and l + 64.

Built like tests/test_gpu_admm_batch.py around the horizon of admm_batch_cases: restart by restart parity with the oracle at NUM_ITERS
= 5 per phase, where tests/test_admm_wide_cpu.py shows the oracle itself stable to 1e-11 on exactly these cases; every exit of the
iteration reached inside that horizon; long runs checked by what does not depend on the last bit (bit-for-bit invariances of the
kernel against itself, the reported values against the returned point, `better` against the start, a median against the project's
serial ADMM path).  The sizes are the smallest at which the wide kernels can go wrong: one, two and 64 live lanes in slot 1, both
sides of the 64 KB LDS image, more restarts than a workgroup has waves, and both ticket regimes."""
import numpy as np
import pytest

import admm_wide_cases as aw
from conftest import oracle_map

pytestmark = pytest.mark.gpu

KEYS = ('iters1', 'iters2', 'f0', 'maxviol', 'X', 'best_index', 'best_f0', 'best_maxviol', 'best_x')


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def make(eng_mod, funcs):
    from qcqp_amd.form import QCQPForm
    return eng_mod.Engine(QCQPForm.from_arrays(funcs))


def host_side(fl, rho=None):
    from qcqp_amd import batch
    P0s, q0s, r0s = aw.objectives(fl)
    m = len(fl[0]) - 1
    rhos = batch.admm_rhos(P0s, m, rho)
    return P0s, q0s, r0s, rhos, batch.admm_minvs(P0s, rhos, m)


def run(eng_mod, fl, R, seed=0, stride=1, fi=0, cons=None, kernel=None, entry='admm_batch_run', **kw):
    """One call on a context built from fl[0]; the dictionary of the call plus rhos and the kernel's name."""
    P0s, q0s, r0s, rhos, Minvs = host_side(fl)
    e = make(eng_mod, fl[0])
    o = getattr(e, entry)(P0s, q0s, r0s, R, rhos, Minvs, seed=seed, seed_stride=stride, first_index=fi, cons=cons, **kw)
    o['kernel'] = e.last_admm_kernel()[0]
    o['rhos'] = rhos
    e.close()
    if kernel is not None:
        assert o['kernel'] == kernel, o['kernel']
    return o


def vs_oracle(orc, fl, o, X0, tag, **kw):
    """Every restart of every problem against improve_admm on the problem's own functions from the same start."""
    B, R, n = X0.shape
    X, i1, i2, f, v = aw.oracle_batch(orc, oracle_map, fl, X0, rhos=o['rhos'], **kw)
    dev = np.array([[aw.rel(o['X'][b, r], X[b, r]) for r in range(R)] for b in range(B)])
    df = float(np.max(np.abs(o['f0'] - f) / (1.0 + np.abs(f))))
    dv = float(np.max(np.abs(o['maxviol'] - v)))
    print('\n%s: %d restarts, point %.1e, f0 %.1e, max violation %.1e; iterations %d..%d + %d..%d'
          % (tag, B * R, dev.max(), df, dv, i1.min(), i1.max(), i2.min(), i2.max()))
    assert np.array_equal(o['iters1'], i1), tag
    assert np.array_equal(o['iters2'], i2), tag
    assert dev.max() < aw.PARITY, (tag, dev.max())
    assert df < aw.PARITY and dv < aw.PARITY, (tag, df, dv)
    return X


def winners_follow(o):
    """best_* are QCQPForm.better folded over the problem's restarts (bucket 1e-4, ties -> lowest index)."""
    for b in range(o['f0'].shape[0]):
        key = sorted((int(v / 1e-4), f, r) for r, (f, v) in enumerate(zip(o['f0'][b], o['maxviol'][b])))[0]
        assert int(o['best_index'][b]) == key[2]
        assert o['best_f0'][b] == o['f0'][b, key[2]] and o['best_maxviol'][b] == o['maxviol'][b, key[2]]
        assert np.array_equal(o['best_x'][b], o['X'][b, key[2]])


@pytest.mark.parametrize('c', aw.cases(), ids=aw.case_id)
def test_every_restart_against_the_oracle(eng_mod, orc, c):
    name, n, B, R, ps, seed, stride, fi = c
    fl = aw.family(name, n, B, seed=ps)
    o = run(eng_mod, fl, R, seed=seed, stride=stride, fi=fi, num_iters=aw.NUM_ITERS,
            kernel='admm_small_kernel<4,w2>' if name in aw.MAXC4 else 'admm_small_kernel<1,w2>')
    vs_oracle(orc, fl, o, aw.starts(orc, seed, stride, fi, B, R, n), aw.case_id(c), num_iters=aw.NUM_ITERS)
    winners_follow(o)


@pytest.mark.parametrize('c', aw.pc_cases(), ids=aw.case_id)
def test_per_problem_coefficients(eng_mod, orc, c):
    name, n, B, R, ps, seed, stride, fi = c
    fl = aw.pc_family(name, n, B, seed=ps)
    o = run(eng_mod, fl, R, seed=seed, stride=stride, fi=fi, cons=aw.cons_of(fl), num_iters=aw.NUM_ITERS,
            kernel='admm_small_kernel<4,pc,w2>' if name in aw.PC_MAXC4 else 'admm_small_kernel<1,pc,w2>')
    vs_oracle(orc, fl, o, aw.starts(orc, seed, stride, fi, B, R, n), aw.case_id(c), num_iters=aw.NUM_ITERS)
    for b in range(B):       # bit for bit the shared call with B = 1 on a context built from problem b's own functions
        o1 = run(eng_mod, [fl[b]], R, seed=aw.seed_of(seed, stride, b), stride=stride, fi=fi, num_iters=aw.NUM_ITERS)
        assert o1['kernel'] in ('admm_small_kernel<1,w2>', 'admm_small_kernel<4,w2>')
        for k in KEYS:
            assert np.array_equal(o[k][b], o1[k][0]), (b, k)


@pytest.mark.parametrize('e', aw.exit_cases(), ids=lambda e: e[0])
def test_every_exit_inside_the_stable_horizon(eng_mod, orc, e):
    label, name, n, ps, kw, want = e
    fl = aw.family(name, n, 2, seed=ps)
    X0, how = aw.exit_starts(orc, e)
    o = run(eng_mod, fl, aw.EXIT_R, **dict(how, **kw))
    assert o['kernel'].endswith('w2>')
    assert want(o['iters1'], o['iters2']), (o['iters1'], o['iters2'])
    vs_oracle(orc, fl, o, X0, label, **kw)


@pytest.mark.parametrize('n,seed', aw.WINNER_CASES)
def test_a_start_that_wins_both_comparisons_comes_back_bit_for_bit(eng_mod, orc, n, seed):
    funcs, x0 = aw.winning_start(orc, n, seed)
    X0 = x0.reshape(1, 1, n)
    o = run(eng_mod, [funcs], 1, X0=X0, kernel='admm_small_kernel<1,w2>', **aw.WINNER_KW)
    vs_oracle(orc, [funcs], o, X0, 'winner', **aw.WINNER_KW)
    assert o['iters1'][0, 0] > 0 and o['iters2'][0, 0] > 0
    assert np.array_equal(o['X'][0, 0], x0)


@pytest.mark.parametrize('n', (33, 64))
def test_old_and_new_symbol_are_the_same_launch_up_to_64(eng_mod, n):
    for name, kernel in (('bls', 'admm_small_kernel<1>'), ('ann2', 'admm_small_kernel<4>')):
        fl = aw.family(name, n, 3, seed=4)
        old = run(eng_mod, fl, 9, seed=5, stride=2, fi=1, num_iters=30, entry='admm_small_batch_run', kernel=kernel)
        new = run(eng_mod, fl, 9, seed=5, stride=2, fi=1, num_iters=30, kernel=kernel)
        for k in KEYS:
            assert np.array_equal(old[k], new[k]), (name, k)
    fl = aw.pc_family('annpp', n, 3, seed=4)
    old = run(eng_mod, fl, 9, seed=5, num_iters=30, cons=aw.cons_of(fl), entry='admm_small_batch_run', kernel='admm_small_kernel<4,pc>')
    new = run(eng_mod, fl, 9, seed=5, num_iters=30, cons=aw.cons_of(fl), kernel='admm_small_kernel<4,pc>')
    for k in KEYS:
        assert np.array_equal(old[k], new[k]), k


def test_invariance_bit_for_bit(eng_mod):
    """num_iters = 40: far beyond the horizon of parity with the oracle -- bits do not care."""
    N = 40
    fl = aw.family('bls', 97, 24, seed=2)
    R = 12
    o = run(eng_mod, fl, R, seed=4, stride=2, num_iters=N, kernel='admm_small_kernel<1,w2>')
    assert o['iters2'].max() > aw.NUM_ITERS
    for b in range(24):                       # a batch of 24 = 24 batches of 1
        o1 = run(eng_mod, [fl[b]], R, seed=4 + 2 * b, stride=2, num_iters=N)
        for k in KEYS:
            assert np.array_equal(o[k][b], o1[k][0]), (b, k)
    perm = np.random.RandomState(0).permutation(24)     # the order of the problems (one seed for all: stride 0)
    oa = run(eng_mod, fl, R, seed=4, stride=0, num_iters=N)
    ob = run(eng_mod, [fl[p] for p in perm], R, seed=4, stride=0, num_iters=N)
    for k in KEYS:
        assert np.array_equal(oa[k][perm], ob[k]), k
    h0 = run(eng_mod, fl, R // 2, seed=4, stride=2, fi=0, num_iters=N)       # R at first_index 0 = R / 2 at 0 and at R / 2
    h1 = run(eng_mod, fl, R // 2, seed=4, stride=2, fi=R // 2, num_iters=N)
    for k in ('iters1', 'iters2', 'f0', 'maxviol', 'X'):
        assert np.array_equal(o[k], np.concatenate([h0[k], h1[k]], axis=1)), k
    # cons repeating the context's coefficients = the shared call
    oc = run(eng_mod, fl, R, seed=4, stride=2, num_iters=N, cons=aw.cons_of(fl), kernel='admm_small_kernel<1,pc,w2>')
    for k in KEYS:
        assert np.array_equal(o[k], oc[k]), k


def test_ticket_is_a_problem_bit_for_bit(eng_mod):
    """B = 300, R = 2 at n = 128: a ticket is a problem.  Restart (b, r) is the restart of the batch of one."""
    N = 40
    many = aw.family('cut', 128, 300, seed=5)
    o = run(eng_mod, many, 2, seed=9, stride=1, num_iters=N, kernel='admm_small_kernel<1,w2>')
    for b in (0, 151, 299):
        o1 = run(eng_mod, [many[b]], 2, seed=9 + b, num_iters=N)
        for k in KEYS:
            assert np.array_equal(o[k][b], o1[k][0]), (b, k)
    winners_follow(o)


def test_ticket_is_a_chunk_of_restarts_bit_for_bit(eng_mod):
    """B = 2, R = 300 at n = 97: a ticket is a chunk of a problem's restarts.  Restart (b, r) is the restart of the batch of one."""
    N = 40
    few = aw.family('ann2', 97, 2, seed=5)
    o = run(eng_mod, few, 300, seed=9, stride=7, num_iters=N, kernel='admm_small_kernel<4,w2>')
    for b in (0, 1):
        parts = [run(eng_mod, [few[b]], 100, seed=9 + 7 * b, fi=fi, num_iters=N) for fi in (0, 100, 200)]
        for k in ('iters1', 'iters2', 'f0', 'maxviol', 'X'):
            assert np.array_equal(o[k][b], np.concatenate([p[k][0] for p in parts], axis=0)), (b, k)
    winners_follow(o)


def test_uploaded_starts(eng_mod, orc):
    n, B, R = 100, 2, 7
    fl = aw.family('box', n, B, seed=8)
    X0 = np.random.RandomState(3).randn(B, R, n)
    o = run(eng_mod, fl, R, X0=X0, num_iters=aw.NUM_ITERS, kernel='admm_small_kernel<1,w2>')
    vs_oracle(orc, fl, o, X0, 'uploaded starts', num_iters=aw.NUM_ITERS)
    for b in range(B):                                      # and restart (b, r) is the restart of the batch of one from the same start
        o1 = run(eng_mod, [fl[b]], R, X0=X0[b:b + 1], num_iters=aw.NUM_ITERS)
        for k in KEYS:
            assert np.array_equal(o[k][b], o1[k][0]), (b, k)


@pytest.mark.parametrize('free', aw.FREE_CASES, ids=lambda f: 'free-' + '-'.join(map(str, f)))
def test_coordinates_without_a_constraint(eng_mod, orc, free):
    """(tests/test_admm_wide_cpu.py asserts that the oracle is stable on these two problems.)"""
    fl = aw.free_family(free, 2)
    o = run(eng_mod, fl, aw.FREE_R, seed=aw.FREE_SEED, stride=3, num_iters=aw.NUM_ITERS, kernel='admm_small_kernel<1,w2>')
    vs_oracle(orc, fl, o, aw.starts(orc, aw.FREE_SEED, 3, 0, 2, aw.FREE_R, aw.FREE_N), 'free %s' % (free,), num_iters=aw.NUM_ITERS)


def serial(eng_mod, funcs, X0, rho, Minv, num_iters):
    """The project's serial ADMM path: a context per problem, pop_upload + admm_run on unit bases with the host inverse."""
    from qcqp_amd.form import QCQPForm
    form = QCQPForm.from_arrays(funcs)
    e = eng_mod.Engine(form)
    e.admm_set_basis(*form.unit_bases())
    e.admm_unit_bases(True)
    e.upload(np.ascontiguousarray(X0.T))
    out = e.admm_run(rho, Minv, phase1=True, num_iters=num_iters)
    X = e.download().T
    e.close()
    return X, out


@pytest.mark.parametrize('name,n', [('bls', 96), ('cut', 128)])
def test_long_runs_without_the_oracle(eng_mod, orc, name, n):
    """num_iters = 200: what does not depend on the last bit.  Against the serial path only the MEDIAN deviation is asserted (1e-6, the
    project's own ADMM figure): no maximum can be derived for a restart whose iteration amplifies rounding for 400 iterations."""
    N, B, R, seed = 200, 2, 16, 12
    fl = aw.family(name, n, B, seed=6)
    P0s, q0s, r0s, rhos, Minvs = host_side(fl)
    o = run(eng_mod, fl, R, seed=seed, num_iters=N, kernel='admm_small_kernel<1,w2>')
    X0 = aw.starts(orc, seed, 1, 0, B, R, n)
    assert (o['iters1'] <= N).all() and (o['iters2'] <= N).all() and (o['iters2'] >= 1).all()
    dev = []
    for b in range(B):
        prob = orc.Problem(fl[b])
        for r in range(R):
            x = o['X'][b, r]
            f, v = prob.eval(0, x), prob.max_violation(x)
            assert abs(o['f0'][b, r] - f) <= 1e-9 * (1 + abs(f)) and abs(o['maxviol'][b, r] - v) <= 1e-9, (b, r)
            # not worse than its start under QCQPForm.better
            f0, v0 = prob.eval(0, X0[b, r]), prob.max_violation(X0[b, r])
            assert int(v / 1e-4) < int(v0 / 1e-4) or (int(v / 1e-4) == int(v0 / 1e-4) and f <= f0), (b, r)
        Xs, so = serial(eng_mod, fl[b], X0[b], float(rhos[b]), Minvs[b], N)
        dev += [aw.rel(o['X'][b, r], Xs[r]) for r in range(R)]
    dev = np.array(dev)
    print('\nlong run %s n=%d, %d + %d iterations: vs the serial path median %.1e max %.1e' % (name, n, N, N, np.median(dev), dev.max()))
    assert np.median(dev) < 1e-6


def test_refusals_leave_the_population_alone(eng_mod):
    from qcqp_amd import problems

    def refused(funcs, code, B=2, R=4, **bad):
        e = make(eng_mod, funcs)
        e.randn(19, seed=3)
        before, kern = e.download(), e.last_cd_kernel()
        n, m = e.n, e.m
        a = dict(P0s=np.zeros((B, n, n)), q0s=np.zeros((B, n)), r0s=np.zeros(B), rhos=np.ones(B), Minvs=np.stack([np.eye(n)] * B) if B else np.zeros((0, n, n)))
        cons = bad.pop('cons', None)
        a.update(bad)
        with pytest.raises(eng_mod.EngineError) as ex:
            e.admm_batch_run(a['P0s'], a['q0s'], a['r0s'], R, a['rhos'], a['Minvs'], num_iters=3, cons=cons(B, m) if cons else None)
        assert ex.value.code == code, (ex.value.code, str(ex.value))
        assert e.pop_size == 19 and np.array_equal(e.download(), before) and e.last_cd_kernel() == kern
        e.close()

    refused(problems.boolean_least_squares(129, 140, seed=1)[0], -4)              # n = 129
    funcs = problems.boolean_least_squares(100, 110, seed=1)[0]
    P = np.zeros((100, 100))
    P[70, 71] = P[71, 70] = 0.5
    refused(funcs + [(P, np.zeros(100), -1.0, '<=')], -4)                         # a coupled constraint
    refused(funcs, -1, B=0)
    refused(funcs, -1, R=0)
    for rho in (0.0, -1.0, np.inf, np.nan):
        refused(funcs, -1, rhos=np.array([1.0, rho]))

    def cons_with(p, q, r):
        def build(B, m):
            c = np.tile(np.array([1.0, 0.0, -1.0]), (B, m, 1))
            c[B - 1, m - 1] = (p, q, r)
            return c
        return build
    refused(funcs, -1, cons=cons_with(np.nan, 0.0, -1.0))
    refused(funcs, -1, cons=cons_with(1.0, np.inf, -1.0))
    refused(funcs, -1, cons=cons_with(0.0, 0.0, -1.0))
    big = problems.boolean_least_squares(128, 130, seed=1)[0]
    asym = np.zeros((2, 128, 128))
    asym[1, 70, 100] = 1.0                                                        # slot 1 of both indices
    refused(big, -1, P0s=asym)                                                    # found while staging
    refused(big, -1, Minvs=np.stack([np.eye(128)] * 2) + asym)


def test_facade(eng_mod):
    from qcqp_amd import settings as s
    from qcqp_amd.batch import QCQPBatch
    B, n, R, seed = 3, 96, 12, 17
    fl = aw.family('bls', n, B, seed=2)
    qb = QCQPBatch(fl)
    with pytest.raises(Exception, match='SDR'):              # suggest(RANDOM) is the only way past n = 64
        qb.suggest(s.SDR, num_samples=R, seed=seed)
    qb.suggest(s.RANDOM, num_samples=R, seed=seed, first_index=3, seed_stride=2)
    with pytest.raises(Exception, match='n <= 64') as ex:
        qb.improve(s.ADMM, num_iters=30)
    assert 'wide=True' in str(ex.value)
    f, v = qb.improve(s.ADMM, num_iters=30, wide=True)
    o = run(eng_mod, fl, R, seed=seed, stride=2, fi=3, num_iters=30)
    assert qb.last_stats['kernel'] == 'admm_small_kernel<1,w2>' and qb.last_stats['method'] == s.ADMM
    assert np.array_equal(qb.last_stats['rho'], o['rhos'])
    assert np.array_equal(f, o['best_f0']) and np.array_equal(v, o['best_maxviol']) and np.array_equal(qb.x, o['best_x'])
    assert np.array_equal(qb.best_index, o['best_index']) and np.array_equal(qb.population_f, o['f0'])
    assert np.array_equal(qb.last_stats['iters1'], o['iters1']) and np.array_equal(qb.last_stats['iters2'], o['iters2'])
    qb.close()
    # n <= 64: wide=True is the default's launch
    fl = aw.family('bls', 16, B, seed=2)
    got = []
    for wide in (False, True):
        qs = QCQPBatch(fl)
        qs.suggest(s.RANDOM, num_samples=R, seed=seed)
        f, v = qs.improve(s.ADMM, num_iters=30, wide=wide)
        assert qs.last_stats['kernel'] == 'admm_small_kernel<1>'
        got.append((f, v, qs.x, qs.population_f, qs.population_v, qs.last_stats['iters1'], qs.last_stats['iters2']))
        qs.close()
    for a, b in zip(*got):
        assert np.array_equal(a, b)
