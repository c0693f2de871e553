"""qcqpmi_cd_batch_run (the wide kernels cd_small_kernel<MAXC[,pc],w2>, csrc/cd_small.hip): B problems of 65 <= n <= 128 variables, R
restarts each, in one launch -- one wavefront per (problem, restart), lane l holds the coordinates l and l + 64.  EVERY restart of
EVERY problem is run to convergence against the fast separable oracle (Problem.improve_cd_sep, pinned to the restatement on these
families at these sizes by tests/test_wide_batch_cpu.py) and checked by life_oracle.check_restart: point 1e-9 relative, every counter
and ran_phase2 equal, both status codes 0, objective 1e-9, max violation 1e-12; and the winner of every problem.  The grid covers
n in {65, 66, 95, 96, 97, 127, 128} (one coordinate in slot 1; around the half; lane 63 without a second coordinate; full), B in
{1, 3, 33} and R in {1, 5, 17} for the eight shared families, and n in {65, 96, 128} for the six families with per-problem
constraint coefficients (the nine (B, R) pairs dealt round-robin, so every family sees every B and every R).  Also: the new symbol
equals the old ones bit for bit at n <= 64, bit-for-bit invariance under the batch size, the order of the problems, a split of the
restarts and both ticket regimes, exact ties, uploaded starts, sweep limits, a restart the reference raises on (in either slot), the
refusals, the QCQPBatch facade.  Without the feature every test fails (the symbol does not exist).  Run with `-m gpu` on an MI355X."""

import numpy as np
import pytest

import small_batch_pc_cases as pc
import wide_batch_cases as wc
from life_oracle import make
from test_gpu_small_batch import COUNTERS, check_vs_oracle, family, objectives, same_as_serial, serial

pytestmark = pytest.mark.gpu

KEYS = COUNTERS + ('f0', 'maxviol', 'X', 'best_index', 'best_f0', 'best_maxviol', 'best_x')


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def run(eng_mod, fl, R, seed=5, stride=1, fi=0, cons=None, entry='cd_batch_run', **kw):
    """The call on a context made from problem 0 (with cons any problem of the list fixes the same structure)."""
    e = make(eng_mod, fl[0])
    P0s, q0s, r0s = objectives(fl)
    o = getattr(e, entry)(P0s, q0s, r0s, R, seed=seed, seed_stride=stride, first_index=fi, cons=cons, **kw)
    o['kernel'] = e.last_cd_kernel()
    e.close()
    return o


def wide_name(maxc4, per_problem):
    return 'cd_small_kernel<%d%s,w2>' % (4 if maxc4 else 1, ',pc' if per_problem else '')


def same_bits(a, ia, b, ib, tag, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k][ia], b[k][ib]), tag + (k,)


# ------------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize('n', wc.NW)
@pytest.mark.parametrize('name', wc.SHARED)
def test_every_restart_of_every_problem_against_the_oracle(eng_mod, orc, name, n):
    B, R, fseed, seed, stride, fi = wc.grid_case(wc.SHARED.index(name), wc.NW.index(n), n)
    fl = family(name, n, B, seed=fseed)
    o = run(eng_mod, fl, R, seed=seed, stride=stride, fi=fi)
    assert o['kernel'] == wide_name(name == 'ann2', False), (name, n, o['kernel'])
    check_vs_oracle(eng_mod, orc, fl, o, R, seed, stride, fi, (name, n, B, R))


@pytest.mark.parametrize('n', wc.NW_PC)
@pytest.mark.parametrize('name', pc.FAMILIES)
def test_per_problem_constraints_against_the_oracle_and_the_problems_own_context(eng_mod, orc, name, n):
    B, R, fseed, seed, stride, fi = wc.grid_case(pc.FAMILIES.index(name), wc.NW.index(n), n)
    fl = pc.family(name, n, B, seed=fseed)
    o = run(eng_mod, fl, R, seed=seed, stride=stride, fi=fi, cons=pc.cons_of(fl))
    assert o['kernel'] == wide_name(name in pc.MAXC4, True), (name, n, o['kernel'])
    check_vs_oracle(eng_mod, orc, fl, o, R, seed, stride, fi, (name, n, B, R))
    for b in range(B):      # bit for bit the shared call with B = 1 on a context made from problem b's own functions
        o1 = run(eng_mod, [fl[b]], R, seed=seed + b * stride, fi=fi)
        assert o1['kernel'] == wide_name(name in pc.MAXC4, False)
        same_bits(o, b, o1, 0, (name, n, b))


# ------------------------------------------------------------------------------------------------- the old symbols, n <= 64
@pytest.mark.parametrize('n', [33, 64])
@pytest.mark.parametrize('name', ['box11', 'ann2', 'boxpp', 'annpp'])
def test_new_symbol_equals_the_old_ones_at_small_n(eng_mod, name, n):
    B, R = 5, 17
    per = name in pc.FAMILIES
    fl = pc.family(name, n, B, seed=9) if per else family(name, n, B)
    cons = pc.cons_of(fl) if per else None
    a = run(eng_mod, fl, R, seed=4, stride=2, fi=3, cons=cons, entry='cd_small_batch_run')
    b = run(eng_mod, fl, R, seed=4, stride=2, fi=3, cons=cons)
    assert a['kernel'] == b['kernel'] == 'cd_small_kernel<%d%s>' % (4 if name in ('ann2', 'annpp') else 1, ',pc' if per else '')
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (name, n, k)


# ------------------------------------------------------------------------------------------------------------------ invariance
def test_invariance_bit_for_bit_at_97(eng_mod):
    n, B, R = 97, 33, 16
    fl = family('box11', n, B)
    o = run(eng_mod, fl, R, seed=4, stride=2)
    assert o['kernel'] == 'cd_small_kernel<1,w2>'
    for b in range(B):                        # a batch of 33 = 33 batches of 1
        same_bits(o, b, run(eng_mod, [fl[b]], R, seed=4 + 2 * b, stride=2), 0, ('one', b))
    perm = np.random.RandomState(0).permutation(B)      # the order of the problems (one seed for all: stride 0)
    oa = run(eng_mod, fl, R, seed=4, stride=0)
    ob = run(eng_mod, [fl[p] for p in perm], R, seed=4, stride=0)
    for k in KEYS:
        assert np.array_equal(oa[k][perm], ob[k]), k
    h0 = run(eng_mod, fl, 8, seed=4, stride=2, fi=0)    # R = 16 at first_index 0 = R = 8 at 0 and at 8
    h1 = run(eng_mod, fl, 8, seed=4, stride=2, fi=8)
    for k in COUNTERS + ('f0', 'maxviol', 'X'):
        assert np.array_equal(o[k], np.concatenate([h0[k], h1[k]], axis=1)), k


def test_whole_problem_tickets_equal_batches_of_one_at_128(eng_mod):
    """B = 300 problems of two restarts: more problems than workgroups, a ticket is a whole problem (the R = 17 cases of the grid
    are dealt in chunks)."""
    n, B, R = 128, 300, 2
    fl = family('bls', n, B)
    o = run(eng_mod, fl, R, seed=4, stride=2, num_iters=200)
    assert o['kernel'] == 'cd_small_kernel<1,w2>' and (o['status1'] == 0).all() and (o['status2'] == 0).all()
    assert o['ran_phase2'][[0, 150, 299]].all()      # (two of the 600 restarts end phase 1 at a fixed point outside the gate, in the oracle too)
    for b in (0, 150, 299):
        same_bits(o, b, run(eng_mod, [fl[b]], R, seed=4 + 2 * b, stride=2, num_iters=200), 0, ('tickets', b))


# ------------------------------------------------------------------------------------------------------------------ edge cases
@pytest.mark.parametrize('n', [80, 128])
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


@pytest.mark.parametrize('phase1', [True, False])
def test_uploaded_starts(eng_mod, orc, phase1):
    n, B, R = 100, 3, 17
    fl = family('bls', n, B)
    rs = np.random.RandomState(5)
    # without phase 1 only a start inside the gate reaches phase 2: signs with a perturbation below viol_tol
    X0 = np.sign(rs.randn(B, R, n)) * (1.0 + 1e-3 * rs.randn(B, R, n)) if not phase1 else rs.randn(B, R, n)
    o = run(eng_mod, fl, R, seed=8, X0=X0, phase1=phase1)
    assert phase1 or ((o['sweeps1'] == 0).all() and (o['ran_phase2'] == 1).all())
    check_vs_oracle(eng_mod, orc, fl, o, R, 8, 1, 0, ('upload', phase1), phase1=phase1, X0=X0)


@pytest.mark.parametrize('iters', [0, 1, 2])
def test_sweep_limits(eng_mod, orc, iters):
    n, B, R = 65, 3, 17
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


@pytest.mark.parametrize('dropped', [(69,), (3, 69)])
def test_a_restart_the_reference_raises_on(eng_mod, dropped):
    """A coordinate without a constraint under phase 1 (python: max() of an empty list, qcqp.py:117): status -3, as qcqpmi_cd_run --
    the coordinate of slot 1 alone, and one in each slot (the highest coordinate's code is reported)."""
    n, B, R = 70, 3, 5
    fl = [[f[0]] + [c for c in f[1:] if pc.entry(c[0], c[1])[0] not in dropped] for f in family('bls', n, B)]
    assert all(len(f) == 1 + n - len(dropped) for f in fl)
    o = run(eng_mod, fl, R, seed=2)
    assert (o['status1'] == -3).all() and (o['status2'] == 0).all() and (o['ran_phase2'] == 0).all()
    assert np.isinf(o['f0']).all() and (o['f0'] > 0).all() and np.isinf(o['maxviol']).all() and (o['maxviol'] > 0).all()


def test_refusals_leave_the_population_alone(eng_mod):
    from qcqp_amd import problems

    def refused(funcs, code, call):
        e = make(eng_mod, funcs)
        e.randn(19, seed=3)
        before = e.download()
        with pytest.raises(eng_mod.EngineError) as ex:
            call(e, e.n)
        assert ex.value.code == code, (ex.value.code, str(ex.value))
        assert e.pop_size == 19 and np.array_equal(e.download(), before)
        e.close()

    def zeros(B):
        return lambda e, n: e.cd_batch_run(np.zeros((B, n, n)), np.zeros((B, n)), np.zeros(B), 4)

    refused(problems.boolean_least_squares(129, 140, seed=1)[0], -4, zeros(2))            # n = 129
    funcs = problems.boolean_least_squares(70, 80, seed=1)[0]
    P = np.zeros((70, 70))
    P[0, 69] = P[69, 0] = 0.5
    refused(funcs + [(P, np.zeros(70), -1.0, '<=')], -4, zeros(2))                         # a coupled constraint
    refused(funcs, -1, zeros(0))                                                           # B = 0

    def asymmetric(e, n):                                                                  # only (70, 100) differs from (100, 70)
        P0s = np.zeros((2, n, n))
        P0s[1, 70, 100] = 1.0
        e.cd_batch_run(P0s, np.zeros((2, n)), np.zeros(2), 4)
    refused(problems.boolean_least_squares(128, 130, seed=1)[0], -1, asymmetric)
    fl = pc.family('boxpp', 70, 2)

    def nan_in_cons(e, n):
        P0s, q0s, r0s = objectives(fl)
        bad = pc.cons_of(fl)
        bad[1, 69, 2] = np.nan
        e.cd_batch_run(P0s, q0s, r0s, 4, cons=bad)
    refused(fl[0], -1, nan_in_cons)


# ---------------------------------------------------------------------------------------------------------------------- facade
def test_facade_equals_qcqp_per_problem(eng_mod):
    from qcqp_amd import QCQP, Problem, problems, settings as s
    from qcqp_amd.batch import QCQPBatch
    B, n, R, seed = 4, 96, 32, 17
    fl = problems.boolean_least_squares_batch(B, n, 144, seed=2)
    qb = QCQPBatch(fl)
    qb.suggest(s.RANDOM, num_samples=R, seed=seed, first_index=3)
    f, v = qb.improve(s.COORD_DESCENT, num_iters=200)
    assert qb.x.shape == (B, n) and qb.population_f.shape == (B, R) and qb.last_stats['kernel'] == 'cd_small_kernel<1,w2>'
    for b in range(B):
        q = QCQP(Problem.from_minimize_form(fl[b]))
        q.suggest(s.RANDOM, num_samples=R, seed=seed + b, first_index=3)
        fb, vb = q.improve(s.COORD_DESCENT, num_iters=200, seed=seed + b, first_index=3, stream=False)
        xb = np.asarray(q.prob.variables()[0].value).ravel()
        assert abs(f[b] - fb) <= 1e-9 * (1 + abs(fb)) and abs(v[b] - vb) <= 1e-12, b
        assert np.max(np.abs(qb.x[b] - xb)) <= 1e-9 * (1.0 + np.max(np.abs(xb))), b
        got, want = int(qb.best_index[b]), int(q.best_index)
        if got != want:      # the rule of same_winner: the serial run itself ended restart `got` at its winner's point
            _, sX, _ = serial(eng_mod, fl[b], R, seed + b, 3, num_iters=200)
            assert np.max(np.abs(sX[:, got] - sX[:, want])) <= 1e-12 * (1.0 + np.max(np.abs(sX[:, want]))), (b, got, want)
    qb.close()


def test_facade_per_problem_constraints_equal_the_engine_call(eng_mod):
    from qcqp_amd import settings as s
    from qcqp_amd.batch import QCQPBatch
    B, n, R, seed = 5, 96, 32, 17
    fl = pc.family('boxpp', n, B, seed=2)
    qb = QCQPBatch(fl)
    assert np.array_equal(qb.cons, pc.cons_of(fl))
    qb.suggest(s.RANDOM, num_samples=R, seed=seed, first_index=3, seed_stride=2)
    f, v = qb.improve(s.COORD_DESCENT, num_iters=200)
    assert qb.last_stats['kernel'] == 'cd_small_kernel<1,pc,w2>' and qb.x.shape == (B, n)
    o = run(eng_mod, fl, R, seed=seed, stride=2, fi=3, cons=pc.cons_of(fl), num_iters=200)
    assert np.array_equal(f, o['best_f0']) and np.array_equal(v, o['best_maxviol']) and np.array_equal(qb.x, o['best_x'])
    assert np.array_equal(qb.best_index, o['best_index'])
    assert np.array_equal(qb.population_f, o['f0']) and np.array_equal(qb.population_v, o['maxviol'])
    for k in COUNTERS:
        assert np.array_equal(qb.last_stats[k], o[k]), k
    assert (v < 1e-2).all()
    qb.close()


def test_facade_sdr_is_refused_past_64(eng_mod):
    from qcqp_amd import problems, settings as s
    from qcqp_amd.batch import QCQPBatch
    qb = QCQPBatch(problems.boolean_least_squares_batch(2, 96, 144, seed=2))
    with pytest.raises(Exception) as ex:
        qb.suggest(s.SDR, num_samples=4, seed=1)
    assert 'SDR' in str(ex.value) and 'n <= 64' in str(ex.value)
    qb.suggest(s.RANDOM, num_samples=4, seed=1)      # the batch itself works
    qb.improve(s.COORD_DESCENT, num_iters=50)
    assert qb.last_stats['kernel'] == 'cd_small_kernel<1,w2>'
    qb.close()
