"""qcqpmi_cd_stream_reserve and qcqpmi_cd_stream_run consume ONE decision (stream_plan, csrc/cd_life_plan.h): on six contexts that take
different branches of it -- three blocks with n a multiple of 16 and not, the least the factored kernel takes with and without its
factor, the round-4 kernel, a zero diagonal -- a run after cd_stream_reserve(K, R) gives bit for bit what a fresh engine's run gives
without the reserve, and the kernel is the one the CPU selftest's table names for the shape (tests/stream_plan_cases.py).  A shape
the plan refuses is refused by the run with QCQPMI_EUNSUPPORTED and nothing of the context is touched.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

from stream_plan_cases import KERNEL_NAMES

pytestmark = pytest.mark.gpu

K, R, ITERS = 2, 20, 50


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def problem(shape):
    """funcs and the objective factor (or None) of a named shape of KERNEL_NAMES"""
    from qcqp_amd import lowrank, problems
    if shape == 'maxcut64':
        return problems.maxcut(64, 0.5, seed=1)[0], None
    n, rows = {'bls48': (48, 12), 'bls40': (40, 10), 'bls128_rank16': (128, 16)}[shape]
    funcs = problems.boolean_least_squares(n, rows, seed=1)[0]
    if shape != 'bls128_rank16':
        return funcs, None
    P0 = funcs[0][0]
    P0 = P0.toarray() if hasattr(P0, 'toarray') else np.asarray(P0)
    L = lowrank.objective_factor(P0, max_rank=16)
    assert L is not None and L.shape == (128, 16)
    return funcs, L


def make(eng_mod, funcs, L, switches):
    from qcqp_amd.form import QCQPForm
    e = eng_mod.Engine(QCQPForm.from_arrays(funcs))
    if L is not None:
        e.cd_set_objective_factor(L)
    e.cd_life_version({'default': 0, 'life_version1': 1, 'life_version3': 3}[switches])
    return e


@pytest.mark.parametrize('shape,switches', sorted(KERNEL_NAMES))
def test_run_after_reserve_equals_run_alone(eng_mod, shape, switches):
    funcs, L = problem(shape)
    outs = []
    for reserve in (True, False):
        e = make(eng_mod, funcs, L, switches)
        if reserve:
            e.cd_stream_reserve(K, R)
        o = e.cd_stream_run(K, R, num_iters=ITERS, seed=77, seed_stride=5, first_index=3, first_stride=1000)
        assert e.last_cd_kernel() == KERNEL_NAMES[(shape, switches)]
        assert e.pop_size == K * R
        o['X'] = e.download()
        outs.append(o)
        e.close()
    a, b = outs
    assert sorted(a) == sorted(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
    assert np.all(np.isfinite(a['f0'])) and np.all(a['status1'] == 0) and np.all(a['status2'] == 0)


def test_refused_shape_leaves_the_context_alone(eng_mod):
    """Coupled constraints: the run refuses before it touches anything -- the resident population keeps its size and its points --
    and a reserve of the same shape still succeeds (population, outputs, winners), after which the run refuses all the same."""
    from qcqp_amd import problems
    from qcqp_amd.form import QCQPForm
    funcs = problems.dense_indefinite(48, 6, seed=7)[0]
    e = eng_mod.Engine(QCQPForm.from_arrays(funcs))
    assert not e.separable
    X0 = np.random.RandomState(2).randn(48, 7)
    e.upload(X0)
    before = e.download()
    for reserved in (False, True):
        if reserved:
            e.cd_stream_reserve(1, 7)
        with pytest.raises(eng_mod.EngineError, match='lifecycle') as ei:
            e.cd_stream_run(K, R, num_iters=ITERS)
        assert ei.value.code == eng_mod.E_UNSUPPORTED
        assert e.pop_size == 7
        assert e.download().tobytes() == before.tobytes()
    e.close()
