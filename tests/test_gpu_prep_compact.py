"""Compact late phase-1 sweeps of cd_life_prep_kernel, and the fast first phase of the band visit's bisection on the GPU.

The prep kernel sweeps a tile of 16 restarts in lockstep; from the first sweep with fewer than 16 unfinished columns it visits the
unfinished columns one after the other with all 256 threads.  A restart needs a second phase-1 sweep exactly when a coordinate has
0 < viol - viol_tol <= tol: the bisection finds no step for it, the sweep moves nothing and the restart fails the gate.  The starts
are uploaded so that the tiles differ: in tile 0 no column needs a second sweep, in tile 1 exactly one does (its stuck coordinate is
the LAST one: the lone real coordinate of the last pair at n = 113), in the last tile every column does -- 8 columns and 8 invalid
slots at R = 40 (compact), 16 columns at R = 48 (a full tile stays in lockstep).  Edge values of viol - viol_tol are spread over the
coordinates: those whose outcome is certain in tiles 0 and 1, those decided by the last bit (viol_tol and tol to within an ulp, a
first midpoint within the guard of 0) in the last tile, whose columns fail the gate either way.

Every output of the default run equals the QCQPMI_L2_PREBUILT=0 run (columns built inside the launch) bit for bit; every restart
matches the oracle; the gate-failing restarts are the planted ones and report 2 phase-1 sweeps."""
import numpy as np
import pytest

from conftest import oracle_map
from life_oracle import check_restart, make, oracle_runs

pytestmark = pytest.mark.gpu

KEYS = ('sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2', 'f0', 'maxviol',
        'best_index', 'best_f0', 'best_maxviol', 'best_x')
TOL = 1e-4
SEED, FIRST = 900, 11
STUCK_COL = 21


def _exactly_at(v):
    """A double x with x * x - 1 == v in floating point (v a power of two: x * x is within an ulp of 1 + v around its root)."""
    x = float(np.sqrt(1.0 + v))
    for _ in range(8):
        x = float(np.nextafter(x, -np.inf))
    for _ in range(17):
        if x * (1.0 * x + 0.0) + -1.0 == v:
            return x
        x = float(np.nextafter(x, np.inf))
    raise AssertionError('no double squares to 1 + %r' % v)


# The equality class x^2 == 1 (`band`): a coordinate with viol - viol_tol = 5e-5, inside (0, tol], finds no step (a slack below 0 is
# not achievable for |f| <= s).  The inequality class x^2 <= 1 (`gen`) achieves every slack > -1, so only a coordinate whose
# violation EQUALS viol_tol stays (no step is tried, and the sweep ends on max viol < viol_tol): viol_tol = 2^-7 and a start that
# squares to 1 + 2^-7 exactly.
VIOL_TOLS = {'bls': 1e-2, 'box': 2.0 ** -7}
STUCKS = {'bls': float(np.sqrt(1.01005)), 'box': _exactly_at(2.0 ** -7)}
STUCK_EXCESS = {'bls': (4e-5, 6e-5), 'box': (-1e-300, 1e-300)}


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


_problems = {}


def problem(fam, n):
    """x_i^2 == 1 (`band` step kind) or x_i^2 <= 1 (`gen`), objective of rank 16 with its factor."""
    if (fam, n) not in _problems:
        from qcqp_amd import lowrank, problems
        if fam == 'bls':
            funcs = problems.boolean_least_squares(n, 16, seed=1)[0]
        else:
            funcs = problems.box_least_squares(n, 16, bound=1.0, seed=1, ridge=0.0)[0]
        P0 = funcs[0][0]
        L = lowrank.objective_factor(P0.toarray() if hasattr(P0, 'toarray') else np.asarray(P0), max_rank=288)
        assert L is not None and L.shape == (n, 16)
        _problems[(fam, n)] = (funcs, L)
    return _problems[(fam, n)]


def slack_excess(fam, X):
    """viol - viol_tol per coordinate, formed as the visit forms it (p = 1, q = 0, r = -1)."""
    f = X * (1.0 * X + 0.0) + -1.0
    return (np.abs(f) if fam == 'bls' else np.maximum(f, 0.0)) - VIOL_TOLS[fam]


def up(v):
    return float(np.nextafter(v, np.inf))


def down(v):
    return float(np.nextafter(v, -np.inf))


def layout(fam, n, R):
    """(n, R) starts and the columns that need a second sweep."""
    VIOL_TOL, STUCK, (elo, ehi) = VIOL_TOLS[fam], STUCKS[fam], STUCK_EXCESS[fam]
    rs = np.random.RandomState(7)
    X0 = 1.5 * rs.randn(n, R)
    e = slack_excess(fam, X0)
    X0[(e > -1e-3) & (e < 1e-3)] = 2.0                 # no accidental coordinate anywhere near the two thresholds
    certain = [1.0, -1.0, 0.0, float(np.sqrt(1.005)), -float(np.sqrt(1.0102)), float(np.sqrt(1.0104)), 3.0, 1e8, -1e100, 1e150,
               float(np.sqrt(0.9898)), -float(np.sqrt(0.98))]
    for i, v in enumerate(certain * 3):
        X0[(11 * i + 2) % (n - 1), (5 * i + 1) % 32] = v          # rows 0 .. n - 2 of tiles 0 and 1
    X0[n - 1, 3] = 1e8                                  # the last coordinate (odd n: the lone one of its pair) moves in tile 0 ...
    X0[n - 1, 19] = -0.25
    last = list(range(32, R))
    a, b, c = float(np.sqrt(1.0 + VIOL_TOL)), float(np.sqrt(1.0 + VIOL_TOL + TOL)), float(np.sqrt(1.0 - VIOL_TOL - TOL))
    decided_by_the_last_bit = [a, up(a), down(a), -a, b, up(b), down(b), -up(b), c, up(c), down(c),
                               float(np.sqrt(1.0 + VIOL_TOL + TOL + 4e-9)), float(np.sqrt(1.0 + VIOL_TOL + TOL - 4e-9)),
                               -float(np.sqrt(1.0 + VIOL_TOL + TOL + 2e-9)), float(np.sqrt(1.0 + VIOL_TOL + TOL - 2e-9)),
                               float(np.sqrt(1.0 + VIOL_TOL + 1e-15)), float(np.sqrt(1.0 - VIOL_TOL - TOL + 4e-9))]
    for i, v in enumerate(decided_by_the_last_bit * 2):
        X0[(13 * i + 5) % n, last[i % len(last)]] = v
    X0[n - 1, last[2]] = up(b)
    # ... and is the stuck one of tile 1's column; every column of the last tile gets one too (placed last: nothing overwrites them)
    X0[n - 1, STUCK_COL] = STUCK
    for c_ in last:
        X0[(3 * c_) % n, c_] = STUCK if c_ % 2 else -STUCK
    need2 = np.zeros(R, dtype=bool)
    need2[STUCK_COL] = True
    need2[last] = True
    # the layout is what it claims to be: outside the last tile only the planted coordinate lies within 1e-6 of (0, tol]
    e = slack_excess(fam, X0[:, :32])
    close = (e > -1e-6) & (e < TOL + 1e-6)
    assert close.sum() == 1 and close[n - 1, STUCK_COL] and elo < e[n - 1, STUCK_COL] < ehi
    e = slack_excess(fam, X0[:, 32:])
    assert ((e > elo) & (e < ehi)).any(axis=0).all()
    return X0, need2


def oracle_results(orc, prob, jobs, iters, vt):
    """life_oracle.oracle_runs, which runs at the default viol_tol; the same tuples at another one."""
    if vt == 1e-2:
        return oracle_runs(orc, prob, jobs, iters)

    def one(job):
        x0, sd, gidx = job
        rng = orc.Rng(orc.RNG_KEYED, sd)
        rng.set_restart(gidx)
        x, s1, s2 = prob.improve_cd_sep(x0, num_iters=iters, viol_tol=vt, tol=TOL, rng=rng)
        return x, s1, s2, prob.eval(0, x), prob.max_violation(x)
    return oracle_map(one, jobs)


def run(eng_mod, monkeypatch, funcs, L, X0, prebuilt, iters, vt):
    monkeypatch.setenv('QCQPMI_L2_PREBUILT', '1' if prebuilt else '0')
    e = make(eng_mod, funcs)
    e.cd_set_objective_factor(L)
    e.upload(X0)
    o = e.cd_stream_run(1, X0.shape[1], generate=False, phase1=True, num_iters=iters, viol_tol=vt, tol=TOL, seed=SEED, seed_stride=1,
                        first_index=FIRST, first_stride=0)
    name = e.last_cd_kernel()
    o['X'] = e.download()
    e.close()
    return o, name


CASES = [
    # family, n, R, num_iters
    ('bls', 128, 40, 1), ('bls', 128, 40, 2), ('bls', 128, 40, 1000),
    ('bls', 113, 40, 1), ('bls', 113, 40, 2), ('bls', 113, 40, 1000),
    ('box', 128, 40, 1), ('box', 128, 40, 2), ('box', 128, 40, 1000),          # the `gen` step kind: p1_class_visit in the compact sweep
    ('bls', 113, 48, 1000),                                                     # a full last tile: its second sweep stays in lockstep
]


@pytest.mark.parametrize('fam,n,R,iters', CASES, ids=['%s-%d-R%d-it%d' % c for c in CASES])
def test_compact_sweeps_vs_in_kernel_build_and_oracle(eng_mod, orc, monkeypatch, fam, n, R, iters):
    funcs, L = problem(fam, n)
    X0, need2 = layout(fam, n, R)
    a, name = run(eng_mod, monkeypatch, funcs, L, X0, True, iters, VIOL_TOLS[fam])
    assert 'factored' in name and (',band,' if fam == 'bls' else ',gen,') in name, name
    b, _ = run(eng_mod, monkeypatch, funcs, L, X0, False, iters, VIOL_TOLS[fam])
    for k in KEYS + ('X',):
        if a[k] is None and b[k] is None:
            continue
        assert np.array_equal(a[k], b[k]), k
    prob = orc.Problem(funcs)
    res = oracle_results(orc, prob, [(X0[:, r], SEED, FIRST + r) for r in range(R)], iters, VIOL_TOLS[fam])
    for r in range(R):
        check_restart(a, a['X'], r, res[r], iters, (fam, n, R, iters))
    failed = ~a['ran_phase2'].astype(bool)
    assert np.array_equal(failed, need2), (np.flatnonzero(failed), np.flatnonzero(need2))
    assert (a['sweeps1'][failed] == min(iters, 2)).all() and (a['sweeps1'][~failed] == 1).all(), a['sweeps1']
