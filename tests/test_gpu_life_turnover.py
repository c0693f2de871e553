"""The turnover pass of the factored lifecycle kernel with prebuilt columns: between two episodes the finished slots are written out
and the free slots refilled in ONE pass (every load requested before any is used, the thread that reads an element of the tile
overwrites it).  QCQPMI_L2_PREBUILT=0 keeps the separate write-out and the in-kernel refill (the reference): the same call must give
the same bits -- points, objective, max violation, every counter, both statuses and the best restart of every population -- and a
handful of restarts of every case is checked against the oracle as well.  The shapes are the smallest at which the pass takes
another path: every slot turning over at once, empty slots and the drain, fewer rows than threads with a padded last block, more
rows of Y than threads, sixteen rows per thread and column (several chunks of loads), the `gen` kind, preloaded beside loading
columns, two tiles per workgroup, resident starts.

The pass runs only in launches with more restarts than slots (a launch that fills its slots once keeps the separate passes), so every
launch here is confined to WGS workgroups through the debug knob of the launch plan: 32 slots (64 with two tiles) for 37 restarts or more."""
import numpy as np
import pytest

from life_oracle import check_restart, oracle_runs, starts

pytestmark = pytest.mark.gpu

KEYS = ('sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2', 'f0', 'maxviol',
        'best_index', 'best_f0', 'best_maxviol', 'best_x', 'X')
SEED, FIRST, FSTRIDE = 900, 11, 50000
WGS = 2                          # workgroups of a launch (debug knob 1024 | limit << 12): fewer slots than restarts in every case
NORC = 5                         # restarts of a case checked against the oracle (spread over its populations)


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


_problems = {}


def problem(fam, n, rows):
    from qcqp_amd import lowrank, problems
    if (fam, n, rows) not in _problems:
        if fam == 'bls':
            funcs = problems.boolean_least_squares(n, rows, seed=1)[0]
        else:
            funcs = problems.box_least_squares(n, rows, bound=1.0, seed=1, ridge=0.0)[0]
        P0 = funcs[0][0]
        P0 = P0.toarray() if hasattr(P0, 'toarray') else np.asarray(P0)
        L = lowrank.objective_factor(P0, max_rank=288)
        assert L is not None and L.shape == (n, rows)
        _problems[(fam, n, rows)] = (funcs, L)
    return _problems[(fam, n, rows)]


def run(eng_mod, monkeypatch, funcs, L, prebuilt, K, R, iters, X0=None, y0max=None, tiles=None, wgs=WGS):
    from qcqp_amd.form import QCQPForm
    for name, val in (('QCQPMI_L2_PREBUILT', None if prebuilt else '0'), ('QCQPMI_L2_Y0_MAX', y0max), ('QCQPMI_L2_TILES', tiles)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    e = eng_mod.Engine(QCQPForm.from_arrays(funcs))
    e.cd_set_objective_factor(L)
    if wgs:
        assert K * R > wgs * 16 * (tiles or 1)
        e.L.qcqpmi_debug_profile(e.h, (1024 | (wgs << 12)) << 4, None)
    if X0 is not None:
        e.upload(X0)
    o = e.cd_stream_run(K, R, generate=X0 is None, phase1=True, num_iters=iters, seed=SEED, seed_stride=1, first_index=FIRST,
                        first_stride=FSTRIDE)
    name = e.last_cd_kernel()
    assert 'factored' in name and (tiles != 2 or '2 tiles' in name), name
    o['X'] = e.download()
    e.close()
    return o


def both(eng_mod, monkeypatch, funcs, L, K, R, iters, **kw):
    """The same call with the turnover pass (the default) and with the in-kernel refill and separate write-out: equal bit for bit."""
    a = run(eng_mod, monkeypatch, funcs, L, True, K, R, iters, **kw)
    b = run(eng_mod, monkeypatch, funcs, L, False, K, R, iters, **kw)
    for k in KEYS:
        if a[k] is None and b[k] is None:
            continue
        assert np.array_equal(a[k], b[k]), k
    return a


def against_oracle(eng_mod, orc, funcs, o, K, R, iters, tag, X0=None):
    prob = orc.Problem(funcs)
    picks = sorted(set(int(k) for k in np.linspace(0, K * R - 1, NORC)))
    jobs = []
    for k in picks:
        p, r = divmod(k, R)
        sd, fi = SEED + p, FIRST + p * FSTRIDE
        x0 = X0[:, k] if X0 is not None else starts(eng_mod, funcs, R, sd, fi)[:, r]
        jobs.append((x0, sd, fi + r))
    res = oracle_runs(orc, prob, jobs, iters)
    for k, rr in zip(picks, res):
        check_restart(o, o['X'], k, rr, iters, tag)


CASES = [
    # family, n, rows of A, K, R, num_iters
    ('bls', 128, 16, 4, 64, 0),              # sweep limit 0: every slot finishes every sweep -- each turnover has 16 columns out and 16 in
    ('bls', 128, 16, 3, 37, 1000),           # K R not a multiple of 16: empty slots, and the drain
    ('bls', 113, 17, 2, 48, 1000),           # n16 = 128 rows for 256 threads, one real coordinate in the padded last block
    ('bls', 640, 288, 2, 48, 1000),          # 32 + 16 RB = 320 rows of `pend` and Y0: more than the threads
    ('bls', 4096, 64, 1, 48, 2),             # 16 rows per thread and column: a column spans a chunk of loads, the first turnover 17 chunks
    ('box', 320, 96, 2, 48, 1000),           # the `gen` step kind, no ridge
]


@pytest.mark.parametrize('fam,n,rows,K,R,iters', CASES, ids=['%s-%d-r%d-K%d-R%d-it%d' % c for c in CASES])
def test_turnover_equals_separate_passes(eng_mod, orc, monkeypatch, fam, n, rows, K, R, iters):
    funcs, L = problem(fam, n, rows)
    a = both(eng_mod, monkeypatch, funcs, L, K, R, iters)
    if iters == 0:
        assert not a['ran_phase2'].any() and not a['sweeps1'].any()
    else:
        assert a['ran_phase2'].any()
    against_oracle(eng_mod, orc, funcs, a, K, R, iters, (fam, n))


def test_turnover_preloaded_beside_loading_columns(eng_mod, orc, monkeypatch):
    """QCQPMI_L2_Y0_MAX=21: restarts 0 .. 20 come with Y0 and pending moves, the others (five of them in the same tile) load."""
    funcs, L = problem('bls', 113, 17)
    a = both(eng_mod, monkeypatch, funcs, L, 2, 48, 1000, y0max=21)
    against_oracle(eng_mod, orc, funcs, a, 2, 48, 1000, 'y0max')


def test_turnover_two_tiles_per_workgroup(eng_mod, orc, monkeypatch):
    """32 slots and 512 threads per workgroup; the same bits as one tile per workgroup in a launch of its own size (one that fills its
    slots once and keeps the separate passes)."""
    funcs, L = problem('bls', 128, 16)
    a = both(eng_mod, monkeypatch, funcs, L, 3, 37, 1000, tiles=2)
    b = run(eng_mod, monkeypatch, funcs, L, True, 3, 37, 1000, wgs=None)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    against_oracle(eng_mod, orc, funcs, a, 3, 37, 1000, 'tiles')


def test_turnover_resident_starts(eng_mod, orc, monkeypatch):
    """generate = 0: the prep kernel runs phase 1 on the uploaded points in place, the turnover copies what it left."""
    funcs, L = problem('bls', 200, 50)
    rs = np.random.RandomState(5)
    X0 = rs.randn(200, 80)
    X0[:, ::4] = np.sign(X0[:, ::4])                 # a quarter of the starts is feasible already
    a = both(eng_mod, monkeypatch, funcs, L, 2, 40, 500, X0=X0)
    assert a['ran_phase2'].any()
    against_oracle(eng_mod, orc, funcs, a, 2, 40, 500, 'resident', X0=X0)
