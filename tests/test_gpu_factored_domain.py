"""The factored instantiation of cd_life_kernel (qcqpmi_cd_set_objective_factor: P0 = L L^T, the kernel carries Y = L^T X) over its
whole domain -- 113 <= n <= 4096 (8 <= NB <= 256 blocks of 16 coordinates), ranks 1 .. 288 (1 .. 18 blocks of 16 rows of Y over three
multiplying waves) -- with EVERY checked restart run to convergence against the fast separable oracle (Problem.improve_cd_sep: the
reference's coordinate descent with incremental bookkeeping, pinned to the restatement by tests/test_oracle_golden.py).
Per restart: point 1e-9, visits / accepted moves of phase 2, both status codes, the sweeps of phase 1 (deviation 4: the kernel stops
a phase 1 that cannot improve, the reference burns its sweeps), objective 1e-9 and max violation 1e-12 against the oracle's
evaluation of its own point (in extended precision where that sum cancels: ExactObjective); per population: the winner the selection rule picks from the oracle's results.
Also: the refusals at the domain's edges, and QCQP.improve's factor switch.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

from life_oracle import ExactObjective, check_restart, make, oracle_runs, oracle_winner, rel, starts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def problem(fam, n, rank):
    """funcs and the factor the API would hand over (P0 = A^T A of rank = rows of A; no ridge)."""
    from qcqp_amd import lowrank, problems
    if fam == 'bls':
        funcs = problems.boolean_least_squares(n, rank, seed=1)[0]
    elif fam == 'box':
        funcs = problems.box_least_squares(n, rank, bound=1.0, seed=1, ridge=0.0)[0]
    elif fam == 'disc':         # x_i^2 <= 0.49: active bounds
        funcs = problems.box_least_squares(n, rank, bound=0.7, seed=5, ridge=0.0)[0]
    else:
        raise KeyError(fam)
    P0 = funcs[0][0]
    L = lowrank.objective_factor(P0.toarray() if hasattr(P0, 'toarray') else np.asarray(P0), max_rank=288)
    assert L is not None and L.shape == (n, rank)
    return funcs, L


def run_factored(eng_mod, funcs, L, K, R, seed0, first0, fstride, iters=1000, X0=None, phase1=True):
    es = make(eng_mod, funcs)
    es.cd_set_objective_factor(L)
    if X0 is not None:
        es.upload(X0)
    o = es.cd_stream_run(K, R, generate=X0 is None, phase1=phase1, num_iters=iters, seed=seed0, seed_stride=1, first_index=first0,
                         first_stride=fstride)
    name = es.last_cd_kernel()
    X = es.download()
    es.close()
    return o, X, name


GRID = [
    # family, n, rank, R per population (K = 2): every restart against the oracle
    ('bls', 113, 16, 256),        # NB = 8, one real coordinate in the last block
    ('bls', 128, 1, 256),         # RB = 1: two of the three multiplying waves own no block of Y
    ('bls', 200, 17, 256),        # the second block of Y holds one row
    ('bls', 1024, 287, 160),      # the largest footprint (RB = 18), last block of Y partial
    ('bls', 1024, 288, 160),      # the largest footprint, 6 + 6 + 6 blocks of Y
    ('bls', 1040, 256, 128),      # the first n that leaves the eight-wave kernel when no factor is set
    ('bls', 1500, 200, 96),       # n not a multiple of 16
    ('bls', 2304, 288, 48),
    ('bls', 2305, 64, 32),        # one real coordinate in block 145
    ('bls', 3001, 150, 32),
    ('bls', 4095, 256, 32),
    ('bls', 4096, 288, 32),       # NB = 256, RB = 18
    ('box', 2320, 200, 32),       # the `gen` step kind past 2304
    ('box', 4096, 96, 32),
    ('disc', 3000, 100, 32),      # active bounds
]


@pytest.mark.parametrize('fam,n,rank,R', GRID, ids=['%s-%d-r%d' % c[:3] for c in GRID])
def test_factored_kernel_domain_vs_oracle(eng_mod, orc, fam, n, rank, R):
    funcs, L = problem(fam, n, rank)
    K, seed0, first0, fstride = 2, 300 + n, 7, 100000
    o, X, name = run_factored(eng_mod, funcs, L, K, R, seed0, first0, fstride)
    assert 'factored' in name and (',band,' if fam == 'bls' else ',gen,') in name, name
    prob, exact = orc.Problem(funcs), ExactObjective(funcs)
    for p in range(K):
        sd, fi = seed0 + p, first0 + p * fstride
        X0 = starts(eng_mod, funcs, R, sd, fi)
        res = oracle_runs(orc, prob, [(X0[:, r], sd, fi + r) for r in range(R)], 1000)
        for r in range(R):
            check_restart(o, X, p * R + r, res[r], 1000, (fam, n, rank, p), exact)
        assert o['best_index'][p] == oracle_winner(res), (fam, n, rank, p)


def test_factored_headline_every_late_refill(eng_mod, orc):
    """BASELINE.json configs[1]'s shape, n = 1024 rank 256, as K = 3 populations of R = 4096: 12 288 restarts, more than the launch has
    slots, so the last population starts in refills late in the launch.  All of the last population and 256 restarts of each of the
    others against the oracle (4608 in all), every restart of the first two against the serial path (which multiplies with P0)."""
    funcs, L = problem('bls', 1024, 256)
    K, R, seed0, first0, fstride = 3, 4096, 41, 0, 4096
    o, X, name = run_factored(eng_mod, funcs, L, K, R, seed0, first0, fstride)
    assert name == 'cd_life_kernel<3,band,factored>', name
    prob = orc.Problem(funcs)
    e = make(eng_mod, funcs)
    for p in range(K):
        sd, fi = seed0 + p, first0 + p * fstride
        sl = slice(p * R, (p + 1) * R)
        e.randn(R, seed=sd, first_index=fi)
        X0 = e.download()
        picks = list(range(R)) if p == K - 1 else list(range(0, R, R // 256))
        res = oracle_runs(orc, prob, [(X0[:, r], sd, fi + r) for r in picks], 1000)
        for r, rr in zip(picks, res):
            check_restart(o, X, p * R + r, rr, 1000, ('headline', p))
        if p == K - 1:
            assert o['best_index'][p] == oracle_winner(res)
        else:
            outr = e.cd_run(phase1=True, num_iters=1000, seed=sd, first_index=fi)
            assert 'factored' not in e.last_cd_kernel()
            assert rel(X[:, sl], e.download()) < 1e-9, p
            for key in ('sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2'):
                assert np.array_equal(o[key][sl], outr[key]), (p, key)
            assert o['best_index'][p] == e.select_best(1e-4)[0], p
    e.close()


@pytest.mark.parametrize('phase1', [True, False])
def test_factored_resident_starts_past_2304(eng_mod, orc, phase1):
    """generate = 0 at n = 2320: phase 1 on the uploaded points in place, or none; near-feasible starts pass the gate, the scaled
    ones do not without phase 1 (their points stay, their objective is reported)."""
    funcs, L = problem('bls', 2320, 200)
    n, K, R = 2320, 2, 32
    rs = np.random.RandomState(11)
    X0 = np.sign(rs.randn(n, K * R)) * (1.0 - 1e-3 * rs.rand(n, K * R))
    far = rs.rand(K * R) < 0.3
    X0[:, far] *= 1.0 + rs.rand(int(far.sum()))
    seed0, first0, fstride = 23, 5, 1000
    o, X, name = run_factored(eng_mod, funcs, L, K, R, seed0, first0, fstride, X0=X0, phase1=phase1)
    assert 'factored' in name, name
    ran = o['ran_phase2'].astype(bool)
    assert ran.any() and (phase1 or (~ran).any())
    if not phase1:
        assert np.array_equal(X[:, ~ran], X0[:, ~ran])
    prob = orc.Problem(funcs)
    for p in range(K):
        sd, fi = seed0 + p, first0 + p * fstride
        res = oracle_runs(orc, prob, [(X0[:, p * R + r], sd, fi + r) for r in range(R)], 1000, phase1=phase1)
        for r in range(R):
            check_restart(o, X, p * R + r, res[r], 1000, ('resident', phase1, p))
        assert o['best_index'][p] == oracle_winner(res), p


@pytest.mark.parametrize('prebuilt', ['1', '0'])
def test_factored_prebuilt_and_in_kernel_columns_vs_oracle(eng_mod, orc, monkeypatch, prebuilt):
    """QCQPMI_L2_PREBUILT=1 (columns built by cd_life_prep_kernel ahead of the launch) and =0 (built inside the launch), each against
    the oracle past 2304 -- not only against each other."""
    monkeypatch.setenv('QCQPMI_L2_PREBUILT', prebuilt)
    funcs, L = problem('bls', 2320, 200)
    K, R, seed0, first0, fstride = 2, 32, 61, 3, 500
    o, X, name = run_factored(eng_mod, funcs, L, K, R, seed0, first0, fstride)
    assert 'factored' in name, name
    prob = orc.Problem(funcs)
    for p in range(K):
        sd, fi = seed0 + p, first0 + p * fstride
        X0 = starts(eng_mod, funcs, R, sd, fi)
        res = oracle_runs(orc, prob, [(X0[:, r], sd, fi + r) for r in range(R)], 1000)
        for r in range(R):
            check_restart(o, X, p * R + r, res[r], 1000, ('prebuilt', prebuilt, p))
        assert o['best_index'][p] == oracle_winner(res), p


def test_factored_refusals_at_the_domain_edges(eng_mod):
    """n = 112 (NB = 7) and rank 289 (19 blocks of Y): cd_set_objective_factor refuses.  n = 4097 (NB = 257) with a factor set:
    cd_stream_run refuses and leaves the resident population as it was."""
    from qcqp_amd import problems
    funcs, L = problem('bls', 112, 16)
    e = make(eng_mod, funcs)
    with pytest.raises(eng_mod.EngineError) as ei:
        e.cd_set_objective_factor(L)
    assert ei.value.code == eng_mod.E_UNSUPPORTED
    e.close()
    funcs, _, info = problems.boolean_least_squares(1024, 289, seed=1)
    e = make(eng_mod, funcs)
    with pytest.raises(eng_mod.EngineError) as ei:
        e.cd_set_objective_factor(np.ascontiguousarray(info['A'].T))       # P0 = A^T A: an exact factor of 289 columns
    assert ei.value.code == eng_mod.E_UNSUPPORTED
    e.close()
    funcs, L = problem('bls', 4097, 64)
    e = make(eng_mod, funcs)
    e.cd_set_objective_factor(L)
    X0 = np.random.RandomState(3).randn(4097, 32)
    e.upload(X0)
    with pytest.raises(eng_mod.EngineError) as ei:
        e.cd_stream_run(2, 16, generate=False, seed=1)
    assert ei.value.code == eng_mod.E_UNSUPPORTED
    assert np.array_equal(e.download(), X0)
    e.close()


def _api_bls(rows):
    from qcqp_amd import problems
    from qcqp_amd.form import QCQPForm
    funcs = problems.boolean_least_squares(1024, rows, seed=2)[0]
    return funcs, QCQPForm.from_arrays(funcs)


def test_api_factor_off_then_on():
    """improve(COORD_DESCENT, factor=False) and then factor=True on the same QCQP: the first runs the kernel that multiplies with P0,
    the second the factored one (the factor is computed the first time it is wanted, not ruled out by an earlier factor=False)."""
    from qcqp_amd import QCQP, COORD_DESCENT, RANDOM
    _, form = _api_bls(256)
    q = QCQP(form)
    q.suggest(RANDOM, num_samples=64, seed=5)
    q.improve(COORD_DESCENT, seed=7, stream=True, factor=False)
    assert q.engine.last_cd_kernel() == 'cd_life_kernel<3,band>'
    q.suggest(RANDOM, num_samples=64, seed=5)
    q.improve(COORD_DESCENT, seed=7, stream=True, factor=True)
    assert q.engine.last_cd_kernel() == 'cd_life_kernel<3,band,factored>'
    q.suggest(RANDOM, num_samples=64, seed=5)
    q.improve(COORD_DESCENT, seed=7, stream=True, factor=False)
    assert q.engine.last_cd_kernel() == 'cd_life_kernel<3,band>'


@pytest.mark.parametrize('rows,kname', [(288, 'cd_life_kernel<3,band,factored>'), (289, 'cd_life_kernel<3,band>')])
def test_api_factor_rank_limit_best_restart_vs_oracle(orc, rows, kname):
    """Through the API (default factor=True): rows = 288 runs factored, rows = 289 falls back to the kernel that multiplies with P0;
    either way the best restart is the one the oracle's results select, with the oracle's point and values."""
    from qcqp_amd import QCQP, COORD_DESCENT, RANDOM
    funcs, form = _api_bls(rows)
    R = 64
    q = QCQP(form)
    q.suggest(RANDOM, num_samples=R, seed=5)
    X0 = q.population()
    f, v = q.improve(COORD_DESCENT, seed=7, stream=True)
    assert q.engine.last_cd_kernel() == kname
    prob = orc.Problem(funcs)
    res = oracle_runs(orc, prob, [(X0[:, r], 7, r) for r in range(R)], 1000)
    w = oracle_winner(res)
    assert q.best_index == w
    x, _, _, f_or, v_or = res[w]
    assert rel(np.array(q.prob.variables()[0].value).ravel(), x) < 1e-9
    assert abs(f - f_or) <= 1e-9 * (1 + abs(f_or)) and abs(v - v_or) <= 1e-12
