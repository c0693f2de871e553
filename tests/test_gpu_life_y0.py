"""Preloaded Y0 = L^T x0 of the factored lifecycle kernel: cd_life_y0_kernel computes it for the restarts the prep kernel built, the refill
copies it and the restart skips its loading sweep.  QCQPMI_L2_Y0_MAX=0 keeps the loading sweep for every restart (the reference), an odd
value inside a tile (21) lets preloaded and loading columns share tiles; all three must agree bit for bit -- points, objective, max
violation, every counter, both statuses and the best restart of every population."""
import numpy as np
import pytest

from life_oracle import check_restart, oracle_runs, oracle_winner, starts

pytestmark = pytest.mark.gpu

KEYS = ('sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2', 'f0', 'maxviol',
        'best_index', 'best_f0', 'best_maxviol', 'best_x')
MODES = (None, '0', '21')        # QCQPMI_L2_Y0_MAX: the default (every restart preloaded), none, the first 21


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def problem(fam, n, rows):
    from qcqp_amd import lowrank, problems
    if fam == 'bls':
        funcs = problems.boolean_least_squares(n, rows, seed=1)[0]
    else:
        funcs = problems.box_least_squares(n, rows, bound=1.0, seed=1, ridge=0.0)[0]
    P0 = funcs[0][0]
    P0 = P0.toarray() if hasattr(P0, 'toarray') else np.asarray(P0)
    L = lowrank.objective_factor(P0, max_rank=288)
    assert L is not None and L.shape == (n, rows)
    return funcs, L


def run(eng_mod, monkeypatch, funcs, L, y0max, K, R, iters, X0=None, phase1=True, dbg=0, seed_stride=1, first_stride=50000, tiles=None):
    from qcqp_amd.form import QCQPForm
    monkeypatch.delenv('QCQPMI_L2_PREBUILT', raising=False)
    if y0max is None:
        monkeypatch.delenv('QCQPMI_L2_Y0_MAX', raising=False)
    else:
        monkeypatch.setenv('QCQPMI_L2_Y0_MAX', y0max)
    if tiles is None:
        monkeypatch.delenv('QCQPMI_L2_TILES', raising=False)
    else:
        monkeypatch.setenv('QCQPMI_L2_TILES', str(tiles))
    e = eng_mod.Engine(QCQPForm.from_arrays(funcs))
    e.cd_set_objective_factor(L)
    if dbg:
        e.L.qcqpmi_debug_profile(e.h, dbg << 4, None)
    if X0 is not None:
        e.upload(X0)
    o = e.cd_stream_run(K, R, generate=X0 is None, phase1=phase1, num_iters=iters, seed=900, seed_stride=seed_stride, first_index=11,
                        first_stride=first_stride)
    name = e.last_cd_kernel()
    assert 'factored' in name and (tiles != 2 or '2 tiles' in name), name
    o['X'] = e.download()
    e.close()
    return o


def same(a, b, keys=KEYS + ('X',)):
    for k in keys:
        if a[k] is None and b[k] is None:
            continue
        assert np.array_equal(a[k], b[k]), k


def three(eng_mod, monkeypatch, funcs, L, K, R, iters, **kw):
    """The same call with the default, without any preload and with 21 preloaded restarts; the default's outputs."""
    outs = [run(eng_mod, monkeypatch, funcs, L, m, K, R, iters, **kw) for m in MODES]
    same(outs[0], outs[1])
    same(outs[2], outs[1])
    return outs[0]


CASES = [
    # family, n, rows of A, K, R, num_iters
    ('bls', 128, 16, 2, 48, 1000),           # NB = 8: Y0 over 6 blocks, 2 pending; RB = 1: two multiplying waves own nothing
    ('bls', 113, 17, 2, 48, 1000),           # one real coordinate in the last block (padding in `pend`); RB = 2 with one real row
    ('bls', 640, 288, 2, 48, 1000),          # RB = 18: six blocks of Y per wave
    ('box', 320, 96, 2, 48, 1000),           # the `gen` step kind, no ridge
    ('bls', 128, 16, 3, 37, 1000),           # K R not a multiple of 16
    ('bls', 128, 16, 2, 48, 0),              # sweep limit 0: every restart fails the gate (frozen sweep on the preloaded Y)
    ('bls', 128, 16, 2, 48, 1),              # sweep limit 1: every restart reaches the limit
]


@pytest.mark.parametrize('fam,n,rows,K,R,iters', CASES, ids=['%s-%d-r%d-K%d-R%d-it%d' % c for c in CASES])
def test_y0_preload_equals_loading_sweep(eng_mod, monkeypatch, fam, n, rows, K, R, iters):
    funcs, L = problem(fam, n, rows)
    a = three(eng_mod, monkeypatch, funcs, L, K, R, iters)
    if iters == 0:
        assert not a['ran_phase2'].any() and not a['sweeps1'].any()
    else:
        assert a['ran_phase2'].any()


def test_y0_two_tiles_per_workgroup(eng_mod, monkeypatch):
    funcs, L = problem('bls', 128, 16)
    a = three(eng_mod, monkeypatch, funcs, L, 2, 48, 1000, tiles=2)
    same(a, run(eng_mod, monkeypatch, funcs, L, '0', 2, 48, 1000))


@pytest.mark.parametrize('phase1', [True, False])
def test_y0_resident_starts(eng_mod, monkeypatch, phase1):
    """generate = 0: phase 1 runs on the uploaded points in place; without phase 1 most restarts fail the gate."""
    funcs, L = problem('bls', 200, 50)
    rs = np.random.RandomState(5)
    X0 = rs.randn(200, 80)
    X0[:, ::4] = np.sign(X0[:, ::4])                 # a quarter of the starts is feasible already (passes the gate)
    a = three(eng_mod, monkeypatch, funcs, L, 2, 40, 500, X0=X0, phase1=phase1)
    assert a['ran_phase2'].any() and (phase1 or not a['ran_phase2'].all())


def test_y0_scheduling_invariance(eng_mod, monkeypatch):
    """K populations vs one, and a launch confined to 3 workgroups (preloaded columns enter tiles whose other slots are mid-restart):
    the same bits whatever the schedule and however many restarts are preloaded."""
    funcs, L = problem('bls', 256, 64)
    ref = run(eng_mod, monkeypatch, funcs, L, '0', 3, 64, 1000, seed_stride=0, first_stride=64)
    keys = ('X', 'f0', 'maxviol', 'sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2')
    for K, R, dbg in ((3, 64, 0), (1, 192, 0), (3, 64, 1024 | (3 << 12))):
        for m in MODES:
            o = run(eng_mod, monkeypatch, funcs, L, m, K, R, 1000, dbg=dbg, seed_stride=0, first_stride=R)
            for k in keys:
                assert np.array_equal(o[k], ref[k]), (K, dbg, m, k)


def test_y0_preload_vs_oracle(eng_mod, orc, monkeypatch):
    """Not only against the loading sweep: every restart of the first case against the oracle, at the factored domain test's tolerances."""
    funcs, L = problem('bls', 128, 16)
    K, R = 2, 48
    o = run(eng_mod, monkeypatch, funcs, L, None, K, R, 1000)
    prob = orc.Problem(funcs)
    for p in range(K):
        sd, fi = 900 + p, 11 + p * 50000
        X0 = starts(eng_mod, funcs, R, sd, fi)
        res = oracle_runs(orc, prob, [(X0[:, r], sd, fi + r) for r in range(R)], 1000)
        for r in range(R):
            check_restart(o, o['X'], p * R + r, res[r], 1000, ('y0', p))
        assert o['best_index'][p] == oracle_winner(res), p
