"""cd_life_kernel's step kind for a diagonal of P0 of MIXED sign (L2_KIND_SGN, csrc/cd_life.h) over its domain -- box-constrained QPs
with an indefinite objective (problems.box_qp), one constraint class with one constraint per coordinate, 33 <= n <= 2304 in all four
geometries cd_life2_config chooses -- with every restart run to convergence against the fast separable oracle
(Problem.improve_cd_sep, pinned to the restatement on this family by tests/test_curvature_oracle_cpu.py) and checked as
tests/test_gpu_life_domain.py checks the other kinds (life_oracle.check_restart: point 1e-9, every counter, both status codes,
objective 1e-9, max violation 1e-12; the winner of each population).  Every case asserts the (nmw, cs, kind) triple of the launch
from the line QCQPMI_L2_DEBUG=1 prints, and the kernel's name.  Also: the two-interval sibling (x_i - lo)(x_i - hi) == 0, resident
starts, sweep limits, scheduling invariance, the serial path on the same restarts, the drop-in API, the refusal that remains
(several classes on such a diagonal) and exact ties.  Before the kind existed, cd_stream_run refused every one of these problems with
E_UNSUPPORTED.  Run with `-m gpu` on an MI355X."""
import re

import numpy as np
import pytest

from life_oracle import ExactObjective, check_restart, make, oracle_runs, oracle_winner, rel, starts

pytestmark = pytest.mark.gpu

SGN = 5                                             # L2_KIND_SGN (csrc/cd_life.h)
COUNTERS = ('sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2')
LAUNCH = re.compile(r'cd_life2_launch: nmw (\d+) cs (\d+) kind (\d+)')


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


@pytest.fixture(autouse=True)
def l2_debug(monkeypatch):
    monkeypatch.setenv('QCQPMI_L2_DEBUG', '1')      # cd_life2_launch prints the geometry it launches on stderr


def geometry(n):
    """(nmw, cs, kind) cd_life2_config chooses for a mixed-sign diagonal of n coordinates (RQ_MAXU = 20 blocks per SIMD)."""
    NB = (n + 15) // 16
    if NB <= 4:
        return 3, 0, SGN
    if NB <= 7:
        return 3, 2, SGN
    if NB <= 64:
        return 3, 4, SGN
    assert NB <= 144, n
    return 7, 4, SGN


def kernel_name(trip):
    return 'cd_life_kernel<%d,sgn>' % trip[0]


DIAG = {
    # the three diagonals: mixed (+/-), mixed with zeros (+/-/0), negative everywhere
    'mixed': dict(),
    'zeros': dict(zero_every=7),
    'zeros9': dict(zero_every=9),
    'negative': dict(diagonal='negative'),
}


def box_qp(n, box, diag, relop='<=', seed=1):
    from qcqp_amd import problems
    funcs, _, info = problems.box_qp(n, seed=seed, lo=box[0], hi=box[1], relop=relop, **DIAG[diag])
    d = info['diag']
    if diag == 'negative':
        assert (d < 0).all()
    else:
        assert (d > 0).any() and (d < 0).any() and (d == 0).any() == (diag != 'mixed')
    return funcs


def launch(eng_mod, capfd, funcs, K, R, seed0, first0, fstride, sstride=1, iters=1000, X0=None, phase1=True, dbg=0):
    """One cd_stream_run on a fresh engine: (outputs, points, kernel name, (nmw, cs, kind) of the launch)."""
    es = make(eng_mod, funcs)
    if dbg:
        es.L.qcqpmi_debug_profile(es.h, dbg << 4, None)
    if X0 is not None:
        es.upload(X0)
    capfd.readouterr()
    o = es.cd_stream_run(K, R, generate=X0 is None, phase1=phase1, num_iters=iters, seed=seed0, seed_stride=sstride,
                         first_index=first0, first_stride=fstride)
    found = LAUNCH.findall(capfd.readouterr().err)
    assert found, 'no cd_life2_launch line on stderr'
    name, X = es.last_cd_kernel(), es.download()
    es.close()
    return o, X, name, tuple(int(v) for v in found[-1])


def check_winner(o, rs, p, R, tag):
    """The winner of population p against the oracle's.  The selection key is (violation bucket, f0, index): where several restarts
    of a population end at the SAME point -- small n: this family's minima are few, and their interior coordinates agree to rounding
    only, unlike the Boolean family's vertices -- their objectives differ in the last bits and the lowest one is a matter of
    rounding.  So: the launch's winner is the selection rule applied to the launch's own outputs, exactly; and it is the oracle's
    winner, or a restart whose oracle run ended at the oracle winner's point (1e-9, the tolerance of the points themselves)."""
    from qcqp_amd import dist
    sl = slice(p * R, (p + 1) * R)
    got, want = int(o['best_index'][p]), oracle_winner(rs)
    assert got == dist.select_best_host(o['f0'][sl], o['maxviol'][sl], 1e-4)[2], tag
    assert got == want or rel(rs[got][0], rs[want][0]) < 1e-9, tag + (got, want, rs[got][3], rs[want][3])


def check_vs_oracle(eng_mod, orc, funcs, o, X, K, R, seed0, first0, fstride, tag, sstride=1, iters=1000, phase1=True, X0=None):
    """EVERY restart of every population against the oracle, on the starts the launch used (keyed normals, or the uploaded X0), and
    the winner of every population.  All oracle runs of the call side by side."""
    prob, exact = orc.Problem(funcs), ExactObjective(funcs)
    jobs = []
    for p in range(K):
        sd, fi = seed0 + p * sstride, first0 + p * fstride
        S = X0[:, p * R:(p + 1) * R] if X0 is not None else starts(eng_mod, funcs, R, sd, fi)
        jobs += [(S[:, r], sd, fi + r) for r in range(R)]
    res = oracle_runs(orc, prob, jobs, iters, phase1=phase1)
    for k, rr in enumerate(res):
        check_restart(o, X, k, rr, iters, tag + (k // R,), exact)
    for p in range(K):
        check_winner(o, res[p * R:(p + 1) * R], p, R, tag + (p,))
    return res


GRID = [
    # n, box, diagonal, R per population (K = 2): both edges of every NB range
    (33, (-1.0, 1.0), 'mixed', 128),         # NB = 3, one real coordinate in the last block: the lowest n the kernel takes
    (64, (0.0, 1.0), 'zeros', 128),          # NB = 4: the last n without a chain share
    (65, (-1.0, 1.0), 'negative', 128),      # NB = 5: the first with a share of two
    (112, (0.0, 1.0), 'mixed', 128),         # NB = 7: the last with a share of two
    (113, (-1.0, 1.0), 'zeros', 128),        # NB = 8: the first with a share of four
    (1000, (0.0, 1.0), 'zeros9', 32),        # n not a multiple of 16 in the four-wave range
    (1024, (-1.0, 1.0), 'mixed', 32),        # NB = 64: the last four-wave n
    (1025, (0.0, 1.0), 'negative', 32),      # NB = 65: the first eight-wave n, not a multiple of 16
    (2000, (-1.0, 1.0), 'zeros', 32),        # BASELINE.json configs[2]'s size
    (2304, (-1.0, 1.0), 'mixed', 24),        # NB = 144: the largest n
]


def test_grid_covers_the_domain():
    """All four geometries at both edges of their NB range; the three diagonals and both boxes."""
    assert {geometry(n)[:2] for n, _, _, _ in GRID} == {(3, 0), (3, 2), (3, 4), (7, 4)}
    assert {(n + 15) // 16 for n, _, _, _ in GRID} >= {3, 4, 5, 7, 8, 64, 65, 144}
    assert {d.rstrip('9') for _, _, d, _ in GRID} == {'mixed', 'zeros', 'negative'}
    assert {b for _, b, _, _ in GRID} == {(-1.0, 1.0), (0.0, 1.0)}
    assert any(n % 16 and n > 1024 for n, _, _, _ in GRID)


@pytest.mark.parametrize('n,box,diag,R', GRID, ids=['%d-%s' % (c[0], c[2]) for c in GRID])
def test_sgn_kernel_domain_vs_oracle(eng_mod, orc, capfd, n, box, diag, R):
    funcs = box_qp(n, box, diag)
    K, seed0, first0, fstride = 2, 700 + n, 3, 100000
    o, X, name, trip = launch(eng_mod, capfd, funcs, K, R, seed0, first0, fstride)
    want = geometry(n)
    assert trip == want and name == kernel_name(want), (trip, want, name)
    assert o['ran_phase2'].any(), 'no restart reached phase 2'
    check_vs_oracle(eng_mod, orc, funcs, o, X, K, R, seed0, first0, fstride, ('box_qp', n, diag))


@pytest.mark.parametrize('n', [200, 1100])
def test_two_interval_constraint(eng_mod, orc, capfd, n):
    """(x_i - lo)(x_i - hi) == 0 on a mixed diagonal with zeros, from keyed normals through phase 1: the feasible set at the slack
    phase 1 leaves is an interval around lo and one around hi.  One four-wave n and one eight-wave n; the boxes [0, 1] and [-1, 1]."""
    funcs = box_qp(n, (0.0, 1.0) if n == 200 else (-1.0, 1.0), 'zeros', relop='==')
    K, R, seed0, first0, fstride = 2, 32, 900 + n, 1, 5000
    o, X, name, trip = launch(eng_mod, capfd, funcs, K, R, seed0, first0, fstride)
    assert trip == geometry(n) and name == kernel_name(trip), (trip, name)
    assert o['ran_phase2'].any() and o['accepted2'].sum() > 0
    check_vs_oracle(eng_mod, orc, funcs, o, X, K, R, seed0, first0, fstride, ('two_intervals', n))


@pytest.mark.parametrize('phase1', [True, False])
@pytest.mark.parametrize('relop', ['<=', '=='])
def test_resident_starts(eng_mod, orc, capfd, relop, phase1):
    """generate = 0 at n = 1100: phase 1 on the uploaded points in place, or none.  Starts near -1 / 1 pass the gate (for the equality
    their violation, about 2e-3, is the slack of phase 2: two intervals of that width, the fast path's two-interval pick); the
    scaled ones do not without phase 1, and their points stay as uploaded."""
    n, K, R = 1100, 2, 32
    funcs = box_qp(n, (-1.0, 1.0), 'zeros', relop=relop)
    rs = np.random.RandomState(17)
    X0 = np.sign(rs.randn(n, K * R)) * (1.0 - 1e-3 * rs.rand(n, K * R))
    far = rs.rand(K * R) < 0.3
    X0[:, far] *= 1.0 + rs.rand(int(far.sum()))
    seed0, first0, fstride = 29, 11, 1000
    o, X, name, trip = launch(eng_mod, capfd, funcs, K, R, seed0, first0, fstride, X0=X0, phase1=phase1)
    assert trip == (7, 4, SGN) and name == 'cd_life_kernel<7,sgn>', (trip, name)
    ran = o['ran_phase2'].astype(bool)
    assert ran.any() and (phase1 or (~ran).any())
    if not phase1:
        assert np.array_equal(X[:, ~ran], X0[:, ~ran])
    check_vs_oracle(eng_mod, orc, funcs, o, X, K, R, seed0, first0, fstride, ('resident', relop, phase1), phase1=phase1, X0=X0)


@pytest.mark.parametrize('iters', [0, 1, 2])
def test_sweep_limits(eng_mod, orc, capfd, iters):
    """num_iters = 0, 1, 2 at n = 1100: restarts that stop at the limit report their objective from a frozen sweep (the frozen sweep
    that evaluates f0 before phase 2 is not one of the counted sweeps)."""
    n, K, R = 1100, 2, 32
    funcs = box_qp(n, (0.0, 1.0), 'zeros')
    seed0, first0, fstride = 71 + iters, 0, 5000
    o, X, name, trip = launch(eng_mod, capfd, funcs, K, R, seed0, first0, fstride, iters=iters)
    assert trip == (7, 4, SGN) and name == 'cd_life_kernel<7,sgn>', (trip, name)
    check_vs_oracle(eng_mod, orc, funcs, o, X, K, R, seed0, first0, fstride, ('limit', iters), iters=iters)


@pytest.mark.parametrize('n', [176, 1100])
def test_scheduling_invariance(eng_mod, capfd, n):
    """The same 72 restarts as three populations of 24, as one population of 72 (same seed, contiguous restart indices) and with the
    launch confined to two workgroups (the debug knob: refills, episodes that begin and end mid-run): bit-identical points,
    objectives, violations and counters."""
    funcs = box_qp(n, (-1.0, 1.0), 'zeros')
    o3, X3, _, t3 = launch(eng_mod, capfd, funcs, 3, 24, 13, 7, 24, sstride=0)
    o1, X1, _, t1 = launch(eng_mod, capfd, funcs, 1, 72, 13, 7, 0, sstride=0)
    o2, X2, _, t2 = launch(eng_mod, capfd, funcs, 1, 72, 13, 7, 0, sstride=0, dbg=1024 | (2 << 12))
    assert t3 == t1 == t2 == geometry(n), (t3, t1, t2)
    assert o1['ran_phase2'].any() and o1['accepted2'].sum() > 0
    for oo, XX in ((o3, X3), (o2, X2)):
        assert np.array_equal(XX, X1)
        for key in COUNTERS + ('f0', 'maxviol'):
            assert np.array_equal(oo[key], o1[key]), key


@pytest.mark.parametrize('n,iters', [(100, 1000), (128, 1000)])
def test_stream_equals_the_serial_path(eng_mod, capfd, n, iters):
    """cd_stream_run against randn + cd_run (cd_phase2_kernel, what every such problem ran before) on the same global restart
    indices, to convergence: all restarts, points 1e-12, every counter equal.  A share of two (n = 100) and of four (n = 128).
    Why no larger n: the two paths sum (P0 x)_i in different orders, and a step to the vertex divides that sum's rounding, about
    1.1e-16 |g_i| with |g_i| ~ sqrt(n) on this family (q0 = sqrt(n) N(0, 1)), by P0[i,i] -- N(0, 1) here, the smallest positive one
    of n / 2 draws about 2.5 / n -- so ONE step can differ by 4.4e-17 n^1.5: 6e-14 at n = 128, 1.6e-12 at n = 1100, where the bound
    of 1e-12 no longer tells an error from rounding (measured there after three sweeps: 1.7e-11 absolute, every counter equal).
    Past n = 128 the kernel is held against the oracle instead (1e-9, every restart: the tests above)."""
    funcs = box_qp(n, (0.0, 1.0), 'zeros')
    K, R, seed0, first0, fstride = 2, 64, 300 + n, 9, 4000
    o, X, name, trip = launch(eng_mod, capfd, funcs, K, R, seed0, first0, fstride, iters=iters)
    assert trip == geometry(n) and name == kernel_name(trip), (trip, name)
    assert o['ran_phase2'].any() and o['accepted2'].sum() > 0
    e = make(eng_mod, funcs)
    for p in range(K):
        sd, fi = seed0 + p, first0 + p * fstride
        e.randn(R, seed=sd, first_index=fi)
        outr = e.cd_run(phase1=True, num_iters=iters, seed=sd, first_index=fi)
        assert e.last_cd_kernel() == 'cd_phase2_kernel'
        Xr = e.download()
        sl = slice(p * R, (p + 1) * R)
        assert rel(X[:, sl], Xr) < 1e-12, (n, p, np.max(np.abs(X[:, sl] - Xr)))
        for key in COUNTERS:
            assert np.array_equal(o[key][sl], outr[key]), (n, p, key)
    e.close()


def test_through_the_api(capfd):
    """suggest(RANDOM, num_samples=R, batches=K) + improve(COORD_DESCENT) runs the K batches through the new kernel, and batch b ends
    exactly where the b-th of K serial suggest + improve(stream=False) calls ends (tests/test_gpu_api.py::
    test_suggest_batches_streams_improve is the template)."""
    from qcqp_amd import QCQP, COORD_DESCENT, RANDOM
    from qcqp_amd.form import QCQPForm
    form = QCQPForm.from_arrays(box_qp(200, (0.0, 1.0), 'zeros'))
    K, R = 3, 40
    q = QCQP(form)
    q.suggest(RANDOM, num_samples=R, batches=K, seed=5)
    capfd.readouterr()
    f, v = q.improve(COORD_DESCENT, seed=7)
    found = LAUNCH.findall(capfd.readouterr().err)
    assert found and tuple(int(t) for t in found[-1]) == (3, 4, SGN), found
    assert q.engine.last_cd_kernel() == 'cd_life_kernel<3,sgn>'
    assert len(q.batch_results) == K
    q2 = QCQP(form)
    serial = []
    for b in range(K):
        q2.suggest(RANDOM, num_samples=R, seed=5, first_index=b * R)
        fb, vb = q2.improve(COORD_DESCENT, seed=7, first_index=b * R, stream=False)
        assert q2.engine.last_cd_kernel() == 'cd_phase2_kernel'
        serial.append((fb, vb, q2.best_index, np.array(q2.prob.variables()[0].value).ravel()))
        assert abs(q.batch_results[b]['f'] - fb) <= 1e-11 * (1 + abs(fb)) and abs(q.batch_results[b]['v'] - vb) <= 1e-12, b
        assert q.batch_results[b]['index'] == q2.best_index, b
    from qcqp_amd.dist import better_key
    w = min(range(K), key=lambda b: better_key(serial[b][0], serial[b][1], b))
    assert abs(f - serial[w][0]) <= 1e-11 * (1 + abs(f)) and abs(v - serial[w][1]) <= 1e-12
    assert np.max(np.abs(np.array(q.prob.variables()[0].value).ravel() - serial[w][3])) < 1e-12


def test_mixed_curvature_with_two_classes_is_still_refused(eng_mod):
    """A mixed diagonal with TWO classes of boxes stays outside the kernel: E_UNSUPPORTED (the message says where such a problem
    runs), and the resident population is bit-identical afterwards."""
    n = 100
    funcs = box_qp(n, (-1.0, 1.0), 'zeros')
    for i in range(1, n, 2):                         # odd coordinates: the box [-0.7, 0.7]
        P, q, r, relop = funcs[1 + i]
        funcs[1 + i] = (P, q, -0.49, relop)
    e = make(eng_mod, funcs)
    X0 = np.random.RandomState(5).randn(n, 32)
    e.upload(X0)
    with pytest.raises(eng_mod.EngineError) as ei:
        e.cd_stream_run(2, 16, generate=False, seed=1)
    assert ei.value.code == eng_mod.E_UNSUPPORTED and 'mixed sign' in str(ei.value), str(ei.value)
    assert e.pop_size == 32 and np.array_equal(e.download(), X0)
    e.cd_run(seed=1)                                 # ... and runs the serial path
    assert e.last_cd_kernel() == 'cd_phase2_kernel'
    e.close()


def _diagonal_ties(n, relop):
    """P0 = diag(d) with dyadic d of BOTH signs and zeros, q = 0, the box [-1, 1]: no off-diagonal term, so the scalar objective of
    every visit is d_i x^2 exactly, in any arithmetic.  d_i < 0: the outermost end points tie.  d_i == 0: the zero objective, a
    uniform draw from the set.  d_i > 0: the vertex 0 is feasible for the box (no tie); for x^2 == 1 the inner end points tie."""
    import scipy.sparse as sp
    d = (1.0 + (np.arange(n) % 7) / 8.0) * np.where(np.arange(n) % 3 == 0, 1.0, -1.0)
    d[4::5] = 0.0
    funcs = [(np.diag(d), np.zeros(n), 0.0, None)]
    for i in range(n):
        funcs.append((sp.csr_matrix(([1.0], ([i], [i])), shape=(n, n)), np.zeros(n), -1.0, relop))
    return funcs


@pytest.mark.parametrize('relop,n', [('==', 100), ('<=', 100), ('==', 1100)])
def test_exact_ties_of_a_diagonal_objective(eng_mod, orc, capfd, relop, n):
    """Exact ties wherever d_i <= 0 (and, for the equality, everywhere): the kernel's secant slope d_i (omid - x_i) + d_i x_i is
    within rounding of 0, far below its near-tie threshold, its generic path recomputes t1 = 2 ((P0 x)_i - P0[i,i] x_i) = 0 and draws
    as the reference does.  Four sweeps (a random walk among equal candidates does not converge), every restart against the oracle."""
    funcs = _diagonal_ties(n, relop)
    K, R, seed0, first0, fstride, iters = 2, 64, 19, 0, 64, 4
    o, X, name, got = launch(eng_mod, capfd, funcs, K, R, seed0, first0, fstride, iters=iters)
    assert got == geometry(n) and name == kernel_name(got), (got, name)
    assert o['accepted2'].sum() > 0.2 * o['visits2'].sum() > 0
    check_vs_oracle(eng_mod, orc, funcs, o, X, K, R, seed0, first0, fstride, ('ties', relop, n), iters=iters)
