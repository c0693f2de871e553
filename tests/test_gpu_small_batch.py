"""qcqpmi_cd_small_batch_run (cd_small_kernel, csrc/cd_small.hip): B small problems (n <= 64) with shared separable constraints, R
restarts each, in one launch.  EVERY restart of EVERY problem is run to convergence against the fast separable oracle
(Problem.improve_cd_sep, pinned to the restatement on these families at these sizes by tests/test_small_batch_cpu.py) and checked
by life_oracle.check_restart: point 1e-9 relative, every counter and ran_phase2 equal, both status codes 0, objective 1e-9, max
violation 1e-12; and the winner of every problem.  The grid covers n in {1, 2, 7, 16, 17, 31, 32, 33, 48, 63, 64}, B in {1, 3, 64}
and R in {1, 17, 64} for every family (every n with every family; the nine (B, R) pairs dealt round-robin over the cases, so every
family sees every B and every R).  Also: exact ties, the serial path on the same restarts, bit-for-bit invariance under the batch
size, the order of the problems and a split of the restarts, uploaded starts, sweep limits, a restart the reference raises on, the
three refusals, the QCQPBatch facade.  Without the feature every test fails (the symbol and the module do not exist).
Run with `-m gpu` on an MI355X.  Running time of the file there: NOT MEASURED yet (no GPU run was obtained when the file was written;
the oracle side -- about 47 k restarts of n <= 64 -- takes under a minute on 16 host cores)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from life_oracle import check_restart, make, oracle_runs, oracle_winner, rel, starts

pytestmark = pytest.mark.gpu

NS = (1, 2, 7, 16, 17, 31, 32, 33, 48, 63, 64)
BR = list(itertools.product((1, 3, 64), (1, 17, 64)))
COUNTERS = ('sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2')
FAMILIES = ('bls', 'box01', 'box11', 'box01neg', 'box11neg', 'eq2', 'ann2', 'cut')


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def family(name, n, B, seed=1):
    """B problems of the family: the same constraints, B objectives."""
    from qcqp_amd import problems
    seeds = [seed + b for b in range(B)]
    if name == 'bls':
        return problems.boolean_least_squares_batch(B, n, n + n // 2 + 1, seed=seed)
    if name == 'box01':
        return problems.box_qp_batch(n, seeds, lo=0.0, hi=1.0)
    if name == 'box11':
        return problems.box_qp_batch(n, seeds, lo=-1.0, hi=1.0)
    if name == 'box01neg':
        return problems.box_qp_batch(n, seeds, lo=0.0, hi=1.0, diagonal='negative')
    if name == 'box11neg':
        return problems.box_qp_batch(n, seeds, lo=-1.0, hi=1.0, diagonal='negative')
    if name == 'eq2':       # (x - lo)(x - hi) == 0: two intervals at the slack phase 1 leaves
        return problems.box_qp_batch(n, seeds, lo=-0.5, hi=1.0, relop='==')
    if name == 'ann2':      # an annulus class (two constraints per coordinate) beside an equality class
        return [problems.multi_class('ann2', n, seed=sd) for sd in seeds]
    if name == 'cut':       # MAXCUT: zero diagonal, weighted edges
        return [problems.maxcut(n, seed=sd, weighted=True)[0] for sd in seeds]
    raise KeyError(name)


def objectives(fl):
    n = int(np.asarray(fl[0][0][1]).size)
    P0s = np.empty((len(fl), n, n))
    for b, f in enumerate(fl):
        P = np.asarray(f[0][0].toarray() if hasattr(f[0][0], 'toarray') else f[0][0], dtype=np.float64)
        P0s[b] = (P + P.T) / 2.
    return P0s, np.array([np.asarray(f[0][1], dtype=np.float64).ravel() for f in fl]), np.array([float(f[0][2]) for f in fl])


def run(eng_mod, fl, R, seed=5, stride=1, fi=0, engine=None, **kw):
    e = engine or make(eng_mod, fl[0])
    P0s, q0s, r0s = objectives(fl)
    o = e.cd_small_batch_run(P0s, q0s, r0s, R, seed=seed, seed_stride=stride, first_index=fi, **kw)
    o['kernel'] = e.last_cd_kernel()
    if engine is None:
        e.close()
    return o


def of_problem(o, b):
    """Problem b's slice in the shape check_restart reads: 1-D arrays over its restarts and points as columns."""
    d = dict((k, o[k][b]) for k in COUNTERS + ('f0', 'maxviol'))
    return d, np.ascontiguousarray(o['X'][b].T)


def batch_starts(eng_mod, fl, R, seed, stride, fi):
    """The keyed normals of every problem (life_oracle.starts, on ONE engine: the draws do not depend on the problem)."""
    e = make(eng_mod, fl[0])
    out = []
    for b in range(len(fl)):
        e.randn(R, seed=seed + b * stride, first_index=fi)
        out.append(e.download())
    e.close()
    return out


def check_vs_oracle(eng_mod, orc, fl, o, R, seed, stride, fi, tag, iters=1000, phase1=True, X0=None):
    from qcqp_amd import dist
    if X0 is not None:
        S = [np.ascontiguousarray(X0[b].T) for b in range(len(fl))]
    elif len(fl) <= 3:
        S = [starts(eng_mod, fl[b], R, seed + b * stride, fi) for b in range(len(fl))]
    else:
        S = batch_starts(eng_mod, fl, R, seed, stride, fi)
    for b, funcs in enumerate(fl):
        prob = orc.Problem(funcs)
        sd = seed + b * stride
        res = oracle_runs(orc, prob, [(S[b][:, r], sd, fi + r) for r in range(R)], iters, phase1=phase1)
        ob, Xb = of_problem(o, b)
        for r, rr in enumerate(res):          # every restart: none is left out
            check_restart(ob, Xb, r, rr, iters, tag + (b,))
        # the winner: the selection rule on the launch's own outputs, exactly; and the oracle's winner or a restart that ended at
        # the oracle winner's point (several restarts of a small problem end at the same point; their objectives differ in the last bits)
        got, want = int(o['best_index'][b]), oracle_winner(res)
        assert got == dist.select_best_host(ob['f0'], ob['maxviol'], 1e-4)[2], tag + (b,)
        assert got == want or rel(res[got][0], res[want][0]) < 1e-9, tag + (b, got, want)
        assert o['best_f0'][b] == ob['f0'][got] and o['best_maxviol'][b] == ob['maxviol'][got], tag + (b,)
        assert np.array_equal(o['best_x'][b], Xb[:, got]), tag + (b,)


@pytest.mark.parametrize('name', FAMILIES)
def test_every_restart_of_every_problem_against_the_oracle(eng_mod, orc, name):
    k0 = FAMILIES.index(name)
    for j, n in enumerate(NS):
        B, R = BR[(k0 + j) % len(BR)]
        fl = family(name, n, B, seed=3 + j)
        o = run(eng_mod, fl, R, seed=11 + j, stride=3, fi=5 * j)
        assert o['kernel'] == ('cd_small_kernel<4>' if name == 'ann2' else 'cd_small_kernel<1>')
        check_vs_oracle(eng_mod, orc, fl, o, R, 11 + j, 3, 5 * j, (name, n, B, R))


@pytest.mark.parametrize('n', [16, 40])
def test_exact_ties(eng_mod, orc, n):
    """A diagonal objective of mixed sign with x_i^2 == 1: the two candidates of every phase-2 visit tie exactly, every visit draws."""
    from qcqp_amd import problems
    cons = problems.boolean_least_squares(n, 2, seed=1)[0][1:]
    fl = []
    for b in range(3):
        d = np.random.RandomState(40 + b).randn(n)
        assert (d > 0).any() and (d < 0).any()
        fl.append([(np.diag(d), np.zeros(n), 0.25 * b, None)] + cons)
    o = run(eng_mod, fl, 17, seed=9, num_iters=40)
    assert (o['ran_phase2'] == 1).all() and (o['accepted2'] > 0).all()
    check_vs_oracle(eng_mod, orc, fl, o, 17, 9, 1, 0, ('ties', n), iters=40)


def serial(eng_mod, funcs, R, seed, fi, X0=None, **kw):
    e = make(eng_mod, funcs)
    if X0 is None:
        e.randn(R, seed=seed, first_index=fi)
    else:
        e.upload(X0)
    o = e.cd_run(seed=seed, first_index=fi, **kw)
    X = e.download()
    best = e.select_best()
    e.close()
    return o, X, best


def same_as_serial(o, b, so, sX, tag):
    ob, Xb = of_problem(o, b)
    assert np.max(np.abs(Xb - sX)) <= 1e-12 * (1.0 + np.max(np.abs(sX))), tag
    for k in COUNTERS:
        assert np.array_equal(ob[k], so[k]), (tag, k)
    assert np.all(np.abs(ob['f0'] - so['f0']) <= 1e-9 * (1 + np.abs(so['f0']))) and np.all(np.abs(ob['maxviol'] - so['maxviol']) <= 1e-12), tag


def same_winner(o, b, best, sX, tag):
    """The same winner as the serial path's select_best = (index, f0, max violation, point).  The winner IS a point: its coordinates
    (1e-12, the tolerance of the points), objective (1e-9) and max violation (1e-12) must be the serial winner's, and the batch's
    index must be the selection rule applied to the batch's own outputs, exactly.  The INDEX equals the serial one unless the
    serial run itself ended several restarts at the winner's point: a box QP of 17 variables has few minima, most restarts leave
    phase 1 with violation 0 and the same feasible set, and e.g. restarts 1, 5, 6 and 15 of problem 0 end within 4.4e-16 of each
    other with objectives one ulp apart (-73.38967837767079 / ...078; the CPU oracle shows the same) -- which of them has the
    lowest LAST BIT of f0 depends on the order of the objective's sum (index order here, matrix-core tiles there), so there the
    index may be any restart whose serial run ended at the serial winner's point (1e-12)."""
    from qcqp_amd import dist
    ob, Xb = of_problem(o, b)
    got, want = int(o['best_index'][b]), int(best[0])
    assert got == dist.select_best_host(ob['f0'], ob['maxviol'], 1e-4)[2], tag
    assert np.max(np.abs(o['best_x'][b] - best[3])) <= 1e-12 * (1.0 + np.max(np.abs(best[3]))), tag + (got, want)
    assert abs(o['best_f0'][b] - best[1]) <= 1e-9 * (1 + abs(best[1])) and abs(o['best_maxviol'][b] - best[2]) <= 1e-12, tag + (got, want)
    assert got == want or np.max(np.abs(sX[:, got] - sX[:, want])) <= 1e-12 * (1.0 + np.max(np.abs(sX[:, want]))), tag + (got, want)


@pytest.mark.parametrize('name,n', [('bls', 32), ('box11', 17), ('ann2', 48)])
def test_equals_the_serial_path(eng_mod, name, n):
    B, R, seed, stride, fi = 64, 17, 21, 5, 7
    fl = family(name, n, B)
    o = run(eng_mod, fl, R, seed=seed, stride=stride, fi=fi)
    for b in (0, 1, 13, 40, 63):
        so, sX, best = serial(eng_mod, fl[b], R, seed + b * stride, fi)
        same_as_serial(o, b, so, sX, (name, n, b))
        same_winner(o, b, best, sX, (name, n, b))


def test_invariance_bit_for_bit(eng_mod):
    fl = family('box11', 31, 64)
    R, keys = 64, COUNTERS + ('f0', 'maxviol', 'X', 'best_index', 'best_f0', 'best_maxviol', 'best_x')
    o = run(eng_mod, fl, R, seed=4, stride=2)
    for b in (0, 7, 63):                      # a batch of 64 = 64 batches of 1
        o1 = run(eng_mod, [fl[b]], R, seed=4 + 2 * b, stride=2)
        for k in keys:
            assert np.array_equal(o[k][b], o1[k][0]), (b, k)
    perm = np.random.RandomState(0).permutation(64)     # the order of the problems (one seed for all: stride 0)
    oa = run(eng_mod, fl, R, seed=4, stride=0)
    ob = run(eng_mod, [fl[p] for p in perm], R, seed=4, stride=0)
    for k in keys:
        assert np.array_equal(oa[k][perm], ob[k]), k
    h0 = run(eng_mod, fl, 32, seed=4, stride=2, fi=0)   # R = 64 at first_index 0 = R = 32 at 0 and at 32
    h1 = run(eng_mod, fl, 32, seed=4, stride=2, fi=32)
    for k in COUNTERS + ('f0', 'maxviol', 'X'):
        assert np.array_equal(o[k], np.concatenate([h0[k], h1[k]], axis=1)), k


@pytest.mark.parametrize('phase1', [True, False])
def test_uploaded_starts(eng_mod, orc, phase1):
    n, B, R = 33, 3, 17
    fl = family('bls', n, B)
    rs = np.random.RandomState(5)
    # without phase 1 only a start inside the gate reaches phase 2: signs with a perturbation below viol_tol
    X0 = np.sign(rs.randn(B, R, n)) * (1.0 + 1e-3 * rs.randn(B, R, n)) if not phase1 else rs.randn(B, R, n)
    o = run(eng_mod, fl, R, seed=8, X0=X0, phase1=phase1)
    assert phase1 or ((o['sweeps1'] == 0).all() and (o['ran_phase2'] == 1).all())
    check_vs_oracle(eng_mod, orc, fl, o, R, 8, 1, 0, ('upload', phase1), phase1=phase1, X0=X0)


@pytest.mark.parametrize('iters', [0, 1, 2])
def test_sweep_limits(eng_mod, orc, iters):
    n, B, R = 17, 3, 17
    fl = family('box11', n, B)
    o = run(eng_mod, fl, R, seed=6, num_iters=iters)
    assert (o['sweeps1'] <= iters).all() and (o['sweeps2'] <= iters).all()
    for b in range(B):
        so, sX, _ = serial(eng_mod, fl[b], R, 6 + b, 0, num_iters=iters)
        same_as_serial(o, b, so, sX, ('iters', iters, b))
        prob = orc.Problem(fl[b])             # the objective is reported at the stopping point
        for r in range(R):
            f = prob.eval(0, o['X'][b, r])
            assert abs(o['f0'][b, r] - f) <= 1e-9 * (1 + abs(f)), (iters, b, r)


def test_a_restart_the_reference_raises_on(eng_mod):
    """A coordinate without a constraint under phase 1 (python: max() of an empty list, qcqp.py:117): status -3, as qcqpmi_cd_run."""
    n, B, R = 16, 3, 5
    fl = [f[:-1] for f in family('bls', n, B)]
    o = run(eng_mod, fl, R, seed=2)
    assert (o['status1'] == -3).all() and (o['status2'] == 0).all() and (o['ran_phase2'] == 0).all()
    assert np.isinf(o['f0']).all() and np.isinf(o['maxviol']).all()
    e = make(eng_mod, fl[0])
    e.randn(R, seed=2)
    with pytest.raises(eng_mod.EngineError) as ex:
        e.cd_run(seed=2)
    assert ex.value.code == -5
    st1, st2 = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
    assert e.L.qcqpmi_cd_status(e.h, st1.ctypes.data_as(C.POINTER(C.c_int)), st2.ctypes.data_as(C.POINTER(C.c_int))) == 0
    assert np.array_equal(st1, o['status1'][0]) and np.array_equal(st2, o['status2'][0])
    e.close()


def test_refusals_leave_the_population_alone(eng_mod):
    from qcqp_amd import problems

    def refused(funcs, B, code):
        e = make(eng_mod, funcs)
        e.randn(19, seed=3)
        before = e.download()
        n = e.n
        with pytest.raises(eng_mod.EngineError) as ex:
            e.cd_small_batch_run(np.zeros((B, n, n)), np.zeros((B, n)), np.zeros(B), 4)
        assert ex.value.code == code, (ex.value.code, str(ex.value))
        assert e.pop_size == 19 and np.array_equal(e.download(), before)
        e.close()

    refused(problems.boolean_least_squares(65, 70, seed=1)[0], 2, -4)            # n = 65
    funcs = problems.boolean_least_squares(16, 20, seed=1)[0]
    P = np.zeros((16, 16))
    P[0, 1] = P[1, 0] = 0.5
    refused(funcs + [(P, np.zeros(16), -1.0, '<=')], 2, -4)                      # a coupled constraint
    refused(funcs, 0, -1)                                                        # B = 0
    e = make(eng_mod, funcs)                                                     # a P0_b that is not symmetric
    P0s = np.zeros((2, 16, 16))
    P0s[1, 2, 3] = 1.0
    with pytest.raises(eng_mod.EngineError) as ex:
        e.cd_small_batch_run(P0s, np.zeros((2, 16)), np.zeros(2), 4)
    assert ex.value.code == -1
    e.close()


def test_api_equals_qcqp_per_problem(eng_mod):
    from qcqp_amd import QCQP, Problem, problems, settings as s
    from qcqp_amd.batch import QCQPBatch
    B, n, R, seed = 4, 24, 32, 17
    fl = problems.boolean_least_squares_batch(B, n, 36, seed=2)
    qb = QCQPBatch(fl)
    qb.suggest(s.RANDOM, num_samples=R, seed=seed, first_index=3)
    f, v = qb.improve(s.COORD_DESCENT, num_iters=200)
    assert qb.x.shape == (B, n) and qb.population_f.shape == (B, R) and qb.last_stats['kernel'] == 'cd_small_kernel<1>'
    for b in range(B):
        q = QCQP(Problem.from_minimize_form(fl[b]))
        q.suggest(s.RANDOM, num_samples=R, seed=seed + b, first_index=3)
        fb, vb = q.improve(s.COORD_DESCENT, num_iters=200, seed=seed + b, first_index=3, stream=False)
        xb = np.asarray(q.prob.variables()[0].value).ravel()
        assert abs(f[b] - fb) <= 1e-9 * (1 + abs(fb)) and abs(v[b] - vb) <= 1e-12 and np.max(np.abs(qb.x[b] - xb)) <= 1e-12, b
        assert int(qb.best_index[b]) == int(q.best_index), b
    qb.close()
