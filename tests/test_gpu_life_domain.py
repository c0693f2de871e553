"""cd_life_kernel WITHOUT an objective factor (the instantiations that multiply with P0) over their whole domain -- 33 <= n <= 2304
(3 <= NB <= 144 blocks of 16 coordinates), one to four constraint classes, one or two constraints per coordinate -- with every
checked restart run to convergence against the fast separable oracle (Problem.improve_cd_sep, pinned to the restatement by
tests/test_oracle_golden.py) and checked as test_gpu_factored_domain.py checks the factored kernel (life_oracle.check_restart:
point 1e-9, phase-2 visits and accepted moves, both status codes, phase-1 sweeps, objective 1e-9, max violation 1e-12; the winner
of each population).

cd_life2_config picks one of four geometries from NB: four-wave workgroups with no chain share (NB 3-4), a share of two blocks
(NB 5-7) or four (NB 8-64), eight-wave workgroups with a share of four (NB 65-144); each for the step kinds BAND, GEN, LIN, GENK and
LINK.  The kernel's name does not show the share, so every case also asserts the (nmw, cs, kind) triple of the launch from the line
QCQPMI_L2_DEBUG=1 prints.  The grid reaches all 20 triples, most at both edges of their NB range.  Also: late refills of the
eight-wave kernel, resident starts past 1024, sweep limits 0 .. 2, scheduling invariance, exact ties (a diagonal objective: every
phase-2 visit draws), the refusals at the domain's edges, and a coordinate without a constraint of its own.  Run with `-m gpu` on an
MI355X."""
import re

import numpy as np
import pytest

from life_oracle import ExactObjective, check_restart, make, oracle_runs, oracle_winner, starts

pytestmark = pytest.mark.gpu

BAND, GEN, LIN, GENK, LINK = 0, 1, 2, 3, 4          # L2_KIND_* (csrc/cd_life.h)
KNAME = {BAND: 'band', GEN: 'gen', LIN: 'lin', GENK: 'gen,classes', LINK: 'lin,classes'}
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


def geometry(n, kind):
    """(nmw, cs, kind) cd_life2_config chooses for a problem of n coordinates without a factor (RQ_MAXU = 20 blocks per SIMD)."""
    NB = (n + 15) // 16
    if NB <= 4:
        return 3, 0, kind
    if NB <= 7:
        return 3, 2, kind
    if NB <= 64:
        return 3, 4, kind
    assert NB <= 144, n
    return 7, 4, kind


def kernel_name(trip):
    return 'cd_life_kernel<%d,%s>' % (trip[0], KNAME[trip[2]])


def family(fam, n, rows=None):
    from qcqp_amd import problems
    if fam == 'bls':            # rows > n: a full-rank objective
        return problems.boolean_least_squares(n, rows, seed=1)[0]
    if fam == 'box':
        return problems.box_least_squares(n, max(4, n // 2), bound=1.0, seed=1)[0]
    if fam == 'disc':           # x_i^2 <= 0.49: active bounds
        return problems.box_least_squares(n, max(4, n // 2), bound=0.7, seed=5)[0]
    if fam == 'maxcutw':        # weighted edges: no exact ties between cuts
        return problems.maxcut(n, 0.5, seed=1, weighted=True)[0]
    return problems.multi_class(fam, n, seed=1)


def launch(eng_mod, capfd, funcs, K, R, seed0, first0, fstride, sstride=1, iters=1000, X0=None, phase1=True):
    """One cd_stream_run on a fresh engine: (outputs, points, kernel name, (nmw, cs, kind) of the launch)."""
    es = make(eng_mod, funcs)
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


def check_vs_oracle(eng_mod, orc, funcs, o, X, K, R, seed0, first0, fstride, tag, sstride=1, iters=1000, phase1=True, X0=None,
                    picks=None):
    """Restarts `picks(p)` (default: all) of every population against the oracle, on the starts the launch used (keyed normals, or
    the uploaded X0); the winner of every population checked in full.  All oracle runs of the call side by side."""
    prob, exact = orc.Problem(funcs), ExactObjective(funcs)
    jobs, where = [], []
    for p in range(K):
        sd, fi = seed0 + p * sstride, first0 + p * fstride
        S = X0[:, p * R:(p + 1) * R] if X0 is not None else starts(eng_mod, funcs, R, sd, fi)
        for r in (range(R) if picks is None else picks(p)):
            jobs.append((S[:, r], sd, fi + r))
            where.append((p, r))
    res = oracle_runs(orc, prob, jobs, iters, phase1=phase1)
    per = {}
    for (p, r), rr in zip(where, res):
        check_restart(o, X, p * R + r, rr, iters, tag + (p,), exact)
        per.setdefault(p, []).append(rr)
    for p, rs in per.items():
        if len(rs) == R:
            assert o['best_index'][p] == oracle_winner(rs), tag + (p,)
    return res


GRID = [
    # kind, family, n, rows of A (bls), R per population (K = 2): every restart against the oracle
    (BAND, 'bls', 33, 20, 128),       # NB = 3, one real coordinate in the last block: the lowest n the kernel takes
    (BAND, 'bls', 64, 40, 128),       # NB = 4: the last n without a chain share
    (BAND, 'bls', 65, 100, 128),      # NB = 5: the first with a share of two; full rank
    (BAND, 'bls', 112, 60, 128),      # NB = 7: the last with a share of two
    (BAND, 'bls', 113, 150, 128),     # NB = 8: the first with a share of four; full rank
    (BAND, 'bls', 1024, 1100, 128),   # NB = 64: the last four-wave n; full rank
    (BAND, 'bls', 1025, 400, 128),    # NB = 65: the first eight-wave n
    (BAND, 'bls', 1700, 1800, 64),    # full rank
    (BAND, 'bls', 2304, 2400, 64),    # NB = 144: the largest n without a factor; full rank
    (GEN, 'box', 48, None, 128),
    (GEN, 'disc', 100, None, 128),
    (GEN, 'box', 1024, None, 32),
    (GEN, 'box', 1025, None, 32),
    (GEN, 'disc', 2000, None, 32),
    (GEN, 'box', 2304, None, 24),
    (LIN, 'maxcutw', 40, None, 128),
    (LIN, 'maxcutw', 100, None, 128),
    (LIN, 'maxcutw', 1024, None, 64),
    (LIN, 'maxcutw', 1025, None, 64),
    (LIN, 'maxcutw', 2000, None, 128),# BASELINE.json configs[2]'s size
    (LIN, 'maxcutw', 2304, None, 64),
    (GENK, 'box3', 50, None, 128),
    (GENK, 'ann2', 80, None, 128),
    (GENK, 'box4', 100, None, 128),   # the class table full at a share of two
    (GENK, 'lin2', 1024, None, 32),
    (GENK, 'box4', 1011, None, 32),   # four classes; the padded coordinates (class 4 on the host) stage as class 0
    (GENK, 'box3', 1025, None, 32),
    (GENK, 'box4', 2300, None, 24),   # four classes past 1024, n not a multiple of 16
    (GENK, 'ann2', 2304, None, 48),
    (GENK, 'lin2', 2304, None, 16),
    (LINK, 'cut4', 48, None, 128),
    (LINK, 'cut2', 100, None, 128),
    (LINK, 'cut4', 1024, None, 64),
    (LINK, 'cut2', 1100, None, 64),
    (LINK, 'cut4', 2299, None, 64),   # four classes, n not a multiple of 16
    (LINK, 'cut2', 2304, None, 48),
]


def test_grid_reaches_every_geometry():
    """All 20 (nmw, cs, kind) instantiations cd_life2_config can choose without a factor; BAND at both ends of every NB range."""
    trips = {geometry(n, k) for k, _, n, _, _ in GRID}
    assert trips == {(w, c, k) for (w, c) in ((3, 0), (3, 2), (3, 4), (7, 4)) for k in KNAME}, trips
    nbs = {((n + 15) // 16, k) for k, _, n, _, _ in GRID}
    assert {(3, BAND), (4, BAND), (5, BAND), (7, BAND), (8, BAND), (64, BAND), (65, BAND), (144, BAND)} <= nbs


@pytest.mark.parametrize('kind,fam,n,rows,R', GRID, ids=['%s-%d' % (c[1], c[2]) for c in GRID])
def test_life_kernel_domain_vs_oracle(eng_mod, orc, capfd, kind, fam, n, rows, R):
    funcs = family(fam, n, rows)
    K, seed0, first0, fstride = 2, 500 + n, 3, 100000
    o, X, name, trip = launch(eng_mod, capfd, funcs, K, R, seed0, first0, fstride)
    want = geometry(n, kind)
    assert trip == want and name == kernel_name(want), (trip, want, name)
    assert o['ran_phase2'].any(), 'no restart reached phase 2'
    check_vs_oracle(eng_mod, orc, funcs, o, X, K, R, seed0, first0, fstride, (fam, n))


def test_eight_wave_late_refills(eng_mod, orc, capfd):
    """Three populations of 2048 at n = 1040: 6144 restarts for 16 x CUs = 4096 slots, so the last population starts in refills late
    in the launch.  All of the last population and 256 evenly spaced restarts of each of the others against the oracle."""
    funcs = family('bls', 1040, 260)
    K, R, seed0, first0, fstride = 3, 2048, 41, 0, 2048
    o, X, name, trip = launch(eng_mod, capfd, funcs, K, R, seed0, first0, fstride)
    assert trip == (7, 4, BAND) and name == 'cd_life_kernel<7,band>', (trip, name)
    check_vs_oracle(eng_mod, orc, funcs, o, X, K, R, seed0, first0, fstride, ('refills',),
                    picks=lambda p: range(R) if p == K - 1 else range(0, R, R // 256))


@pytest.mark.parametrize('phase1', [True, False])
@pytest.mark.parametrize('fam,kind', [('bls', BAND), ('ann2', GENK)])
def test_eight_wave_resident_starts(eng_mod, orc, capfd, fam, kind, phase1):
    """generate = 0 at n = 1100: phase 1 on the uploaded points in place, or none.  Near-feasible starts pass the gate; the scaled
    ones do not without phase 1, and their points stay as uploaded."""
    n, K, R = 1100, 2, 32
    funcs = family(fam, n, 300)
    rs = np.random.RandomState(17)
    X0 = np.sign(rs.randn(n, K * R)) * (1.0 - 1e-3 * rs.rand(n, K * R))
    far = rs.rand(K * R) < 0.3
    X0[:, far] *= 1.0 + rs.rand(int(far.sum()))
    seed0, first0, fstride = 29, 11, 1000
    o, X, name, trip = launch(eng_mod, capfd, funcs, K, R, seed0, first0, fstride, X0=X0, phase1=phase1)
    assert trip == (7, 4, kind) and name == kernel_name(trip), (trip, name)
    ran = o['ran_phase2'].astype(bool)
    assert ran.any() and (phase1 or (~ran).any())
    if not phase1:
        assert np.array_equal(X[:, ~ran], X0[:, ~ran])
    check_vs_oracle(eng_mod, orc, funcs, o, X, K, R, seed0, first0, fstride, ('resident', fam, phase1), phase1=phase1, X0=X0)


@pytest.mark.parametrize('iters', [0, 1, 2])
@pytest.mark.parametrize('fam,kind', [('maxcutw', LIN), ('box4', GENK)])
def test_eight_wave_sweep_limits(eng_mod, orc, capfd, fam, kind, iters):
    """num_iters = 0, 1, 2 at n = 1100: restarts that stop at the limit report their objective from a frozen sweep."""
    n, K, R = 1100, 2, 32
    funcs = family(fam, n)
    seed0, first0, fstride = 71 + iters, 0, 5000
    o, X, name, trip = launch(eng_mod, capfd, funcs, K, R, seed0, first0, fstride, iters=iters)
    assert trip == (7, 4, kind) and name == kernel_name(trip), (trip, name)
    check_vs_oracle(eng_mod, orc, funcs, o, X, K, R, seed0, first0, fstride, ('limit', fam, iters), iters=iters)


@pytest.mark.parametrize('fam,rows,kind', [('bls', 260, BAND), ('box', None, GEN), ('maxcutw', None, LIN), ('box4', None, GENK),
                                           ('cut4', None, LINK)])
def test_eight_wave_scheduling_invariance(eng_mod, capfd, fam, rows, kind):
    """The same 72 restarts at n = 1100 as three populations of 24 and as one population of 72 (same seed, contiguous restart
    indices): bit-identical points, objectives, violations and counters."""
    n = 1100
    funcs = family(fam, n, rows)
    o3, X3, _, t3 = launch(eng_mod, capfd, funcs, 3, 24, 13, 7, 24, sstride=0)
    o1, X1, _, t1 = launch(eng_mod, capfd, funcs, 1, 72, 13, 7, 0, sstride=0)
    assert t3 == t1 == (7, 4, kind), (t3, t1)
    assert np.array_equal(X3, X1)
    for key in COUNTERS + ('f0', 'maxviol'):
        assert np.array_equal(o3[key], o1[key]), key


def _diagonal_ties(n, kind):
    """P0 = diag(d) with dyadic d, q = 0: the scalar objective of every visit has t1 = 0 EXACTLY in any arithmetic (no off-diagonal
    term), so its candidate end points tie and the reference draws among them (utilities.py:275-288).  kind 'bls': x_i^2 == 1;
    'ann': the annulus pair on even i beside x_i^2 == 1 on odd i (two classes)."""
    import scipy.sparse as sp
    d = 1.0 + (np.arange(n) % 7) / 8.0
    funcs = [(np.diag(d), np.zeros(n), 0.0, None)]
    for i in range(n):
        P = sp.csr_matrix(([1.0], ([i], [i])), shape=(n, n))
        if kind == 'bls' or i % 2:
            funcs.append((P, np.zeros(n), -1.0, '=='))
        else:
            funcs.append((P, np.zeros(n), -1.0, '<='))
            funcs.append((-P, np.zeros(n), 0.25, '<='))
    return funcs


@pytest.mark.parametrize('kind,n,trip', [('bls', 100, (3, 2, BAND)), ('bls', 1100, (7, 4, BAND)), ('ann', 1100, (7, 4, GENK))])
def test_exact_ties_of_a_diagonal_objective(eng_mod, orc, capfd, kind, n, trip):
    """Every phase-2 visit an exact tie: the kernel's vertex lands within its near-tie threshold, its generic path recomputes
    t1 = 2 ((P0 x)_i - P0[i,i] x_i) = 0 and draws as the reference does.  Four sweeps (a random walk among equal candidates does
    not converge), every restart against the oracle.  A step whose diagonal term is off by one part in 1e12 breaks the tie."""
    funcs = _diagonal_ties(n, kind)
    K, R, seed0, first0, fstride, iters = 2, 64, 19, 0, 64, 4
    o, X, name, got = launch(eng_mod, capfd, funcs, K, R, seed0, first0, fstride, iters=iters)
    assert got == trip and name == kernel_name(trip), (got, name)
    assert o['accepted2'].sum() > 0.3 * o['visits2'].sum() > 0
    check_vs_oracle(eng_mod, orc, funcs, o, X, K, R, seed0, first0, fstride, ('ties', kind, n), iters=iters)


def _bls_with(n, extra):
    """Boolean least squares of n coordinates whose constraint list is rebuilt by extra(i) -> [(p, q, r, relop), ...] per coordinate."""
    import scipy.sparse as sp
    funcs = [family('bls', n, max(4, n // 4))[0]]
    for i in range(n):
        for p, q, r, relop in extra(i):
            qv = np.zeros(n)
            qv[i] = q
            funcs.append((sp.csr_matrix(([float(p)], ([i], [i])), shape=(n, n)), qv, float(r), relop))
    return funcs


REFUSED = {
    'n32': lambda: family('bls', 32, 16),                  # NB = 2
    'n2305': lambda: family('bls', 2305, 64),              # NB = 145 without a factor
    'five_classes': lambda: _bls_with(1500, lambda i: [(1.0, 0.0, -(1.0, 0.81, 0.64, 0.49, 0.36)[i % 5], '<=')]),
    'three_per_coordinate': lambda: _bls_with(1100, lambda i: [(1.0, 0.0, -1.0, '<='), (-1.0, 0.0, 0.25, '<='), (0.0, 1.0, -0.9, '<=')]),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_stream_run_refuses_outside_the_domain(eng_mod, case):
    """n = 32, n = 2305 without a factor, exactly five classes, three constraints per coordinate: E_UNSUPPORTED, and the resident
    population is bit-identical afterwards."""
    funcs = REFUSED[case]()
    n = funcs[0][1].shape[0]
    e = make(eng_mod, funcs)
    X0 = np.random.RandomState(5).randn(n, 32)
    e.upload(X0)
    with pytest.raises(eng_mod.EngineError) as ei:
        e.cd_stream_run(2, 16, seed=1)
    assert ei.value.code == eng_mod.E_UNSUPPORTED, case
    assert e.pop_size == 32 and np.array_equal(e.download(), X0), case
    e.close()


@pytest.mark.parametrize('phase1', [False, True])
def test_coordinate_without_a_constraint_beside_constrained_ones(eng_mod, orc, capfd, phase1):
    """Boolean least squares at n = 100 with the constraint of coordinate 37 removed: two classes among the real coordinates (x^2 == 1
    and no constraint at all), so the GENK kind at a share of two, not a refusal.  The reference's phase 2 minimises over the whole
    line there: without phase 1, every restart against the oracle.  Its phase 1 raises at such a coordinate (max() of an empty
    list): with phase 1, the oracle fails every restart with -3, and so does the launch -- every restart reports status -3 and the
    call fails with QCQPMI_EREFERENCE, as the reference's improve() would."""
    n, K, R = 100, 2, 32
    funcs = family('bls', n, 60)
    del funcs[1 + 37]
    rs = np.random.RandomState(23)
    X0 = np.sign(rs.randn(n, K * R)) * (1.0 - 1e-3 * rs.rand(n, K * R))
    seed0, first0, fstride = 5, 0, 100
    if not phase1:
        o, X, name, trip = launch(eng_mod, capfd, funcs, K, R, seed0, first0, fstride, X0=X0, phase1=False)
        assert trip == (3, 2, GENK) and name == 'cd_life_kernel<3,gen,classes>', (trip, name)
        assert o['ran_phase2'].all()
        check_vs_oracle(eng_mod, orc, funcs, o, X, K, R, seed0, first0, fstride, ('unconstrained',), phase1=False, X0=X0)
        return
    prob = orc.Problem(funcs)
    for k in range(K * R):
        rng = orc.Rng(orc.RNG_KEYED, seed0 + k // R)
        rng.set_restart(first0 + (k // R) * fstride + k % R)
        with pytest.raises(RuntimeError, match='rc=-3'):
            prob.improve_cd_sep(X0[:, k], num_iters=1000, rng=rng)
    e = make(eng_mod, funcs)
    e.upload(X0)
    capfd.readouterr()
    with pytest.raises(eng_mod.EngineError) as ei:
        e.cd_stream_run(K, R, generate=False, phase1=True, seed=seed0, seed_stride=1, first_index=first0, first_stride=fstride)
    assert ei.value.code == -5 and 'appears in no constraint' in str(ei.value), (ei.value.code, str(ei.value))   # QCQPMI_EREFERENCE
    assert [tuple(int(v) for v in t) for t in LAUNCH.findall(capfd.readouterr().err)] == [(3, 2, GENK)]
    e.close()
