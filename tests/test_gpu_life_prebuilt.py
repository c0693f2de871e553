"""Prebuilt columns of the factored lifecycle kernel: cd_life_prep_kernel builds every restart's column ahead of the launch (start
point, phase 1, slack, gate) and the refill only copies it.  QCQPMI_L2_PREBUILT=0 forces the build inside the launch, as before; the
two must agree bit for bit -- points, objective, max violation, every counter and the best restart of every population."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ('sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2', 'f0', 'maxviol',
        'best_index', 'best_f0', 'best_maxviol', 'best_x')


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
    assert L is not None
    return funcs, L


def run(eng_mod, monkeypatch, funcs, L, prebuilt, K, R, iters, X0=None, phase1=True, dbg=0, seed_stride=1, first_stride=50000):
    from qcqp_amd.form import QCQPForm
    monkeypatch.setenv('QCQPMI_L2_PREBUILT', '1' if prebuilt else '0')
    e = eng_mod.Engine(QCQPForm.from_arrays(funcs))
    e.cd_set_objective_factor(L)
    if dbg:
        e.L.qcqpmi_debug_profile(e.h, dbg << 4, None)
    if X0 is not None:
        e.upload(X0)
    o = e.cd_stream_run(K, R, generate=X0 is None, phase1=phase1, num_iters=iters, seed=900, seed_stride=seed_stride, first_index=11,
                        first_stride=first_stride)
    assert 'factored' in e.last_cd_kernel(), e.last_cd_kernel()
    o['X'] = e.download()
    return o


def same(a, b):
    for k in KEYS + ('X',):
        if a[k] is None and b[k] is None:
            continue
        assert np.array_equal(a[k], b[k]), k


CASES = [
    # family, n, rows of A, K, R, num_iters
    ('bls', 128, 32, 2, 600, 1000),          # refills, episodes that begin and end mid-run
    ('bls', 1000, 250, 2, 64, 1000),         # n not a multiple of 16
    ('bls', 1024, 256, 2, 512, 1000),        # the headline shape
    ('bls', 2320, 200, 1, 24, 2),            # past 2304
    ('box', 320, 96, 2, 100, 60),            # the `gen` step kind
    ('bls', 128, 32, 3, 37, 1000),           # K R not a multiple of 16
    ('bls', 128, 32, 2, 48, 0),              # sweep limit 0: no phase 1, every restart fails the gate (frozen sweep)
    ('bls', 256, 64, 2, 48, 1),              # sweep limit 1
]


@pytest.mark.parametrize('fam,n,rows,K,R,iters', CASES, ids=['%s-%d-K%d-R%d-it%d' % (c[0], c[1], c[3], c[4], c[5]) for c in CASES])
def test_prebuilt_equals_in_kernel_build(eng_mod, monkeypatch, fam, n, rows, K, R, iters):
    funcs, L = problem(fam, n, rows)
    a = run(eng_mod, monkeypatch, funcs, L, True, K, R, iters)
    b = run(eng_mod, monkeypatch, funcs, L, False, K, R, iters)
    same(a, b)
    if iters == 0:
        assert not a['ran_phase2'].any() and not a['sweeps1'].any()


@pytest.mark.parametrize('phase1', [True, False])
def test_prebuilt_resident_starts(eng_mod, monkeypatch, phase1):
    """generate = 0: phase 1 runs on the uploaded points in place; without phase 1 most restarts fail the gate."""
    funcs, L = problem('bls', 200, 50)
    rs = np.random.RandomState(5)
    X0 = rs.randn(200, 80)
    X0[:, ::4] = np.sign(X0[:, ::4])                 # a quarter of the starts is feasible already (passes the gate)
    a = run(eng_mod, monkeypatch, funcs, L, True, 2, 40, 500, X0=X0, phase1=phase1)
    b = run(eng_mod, monkeypatch, funcs, L, False, 2, 40, 500, X0=X0, phase1=phase1)
    same(a, b)
    assert a['ran_phase2'].any() and (phase1 or not a['ran_phase2'].all())


def test_prebuilt_scheduling_invariance(eng_mod, monkeypatch):
    """K populations vs one, and a launch confined to 3 workgroups: the same bits with prebuilt columns."""
    funcs, L = problem('bls', 256, 64)
    ref = run(eng_mod, monkeypatch, funcs, L, True, 3, 64, 1000, seed_stride=0, first_stride=64)
    for K, R, dbg in ((1, 192, 0), (3, 64, 1024 | (3 << 12))):
        o = run(eng_mod, monkeypatch, funcs, L, True, K, R, 1000, dbg=dbg, seed_stride=0, first_stride=R)
        for k in ('X', 'f0', 'maxviol', 'sweeps1', 'sweeps2', 'visits2', 'accepted2', 'ran_phase2', 'status1', 'status2'):
            assert np.array_equal(o[k], ref[k]), (K, dbg, k)
