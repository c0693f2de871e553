"""qcqpmi_sdr_solve_unitdiag (sdr_mixing_kernel, csrc/sdr_solve.h; Engine.sdr_solve_unitdiag, the solver behind suggest(SDR) for the
x_i^2 == d_i family up to N = n + 1 = 4096) followed SWEEP BY SWEEP over its domain.  The kernel is a sequential, deterministic chain,
so from a given V0 after T sweeps its V and its history must equal a plain restatement (sdr_mixing_cases.mixing_reference, held to a
long double run of itself in tests/test_sdr_mixing_cpu.py) to rounding: 1e-12 in V and 1e-12 (1 + |f|) in every history entry --
400 times the largest drift between two summation orders in float64 (2.3e-15 at N = 4096) and ten orders below the effect of one lost
or doubled term C_ij v_j (1 / sqrt(N), 1.6e-2 at N = 4096).  The grid (49 cases): dense Gaussian / lifted Boolean least squares /
lifted weighted MAXCUT with an isolated vertex, N in {2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320, 321, 513, 1025, 2049,
4095, 4096} -- register slots q >= 2, the second and later groups of the unrolled product loop, ragged last slots and their clamped
loads, odd N (the row buffers swap between passes), the 64 KB LDS image.  Also: the stop rule and the jump to the last pass (sweep
count, the recomputed last entry, the rest of the history buffer left alone), max_sweeps = 0, a cost that moves no row, bit-for-bit
determinism across calls and contexts, solve_sdr to convergence at n = 256 and n = 300 against the restatement run to the same
tolerance, the five refusals.
Measured on the MI355X (profiles/r20_sdr_mixing_domain.md): see there for the largest deviation per N.
Run with `-m gpu` on an MI355X."""
import ctypes
import functools

import numpy as np
import pytest

import sdr_mixing_cases as mc
from life_oracle import make

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SENTINEL = -7.25e77


@pytest.fixture(scope='module')
def eng_mod():
    from qcqp_amd import engine
    assert engine.device_count() >= 1, 'no HIP device visible'
    return engine


def context(eng_mod):
    """The solver reads nothing of the context's own problem: any small one serves."""
    from qcqp_amd import problems
    return make(eng_mod, problems.boolean_least_squares(4, 6, seed=1)[0])


@pytest.fixture(scope='module')
def ctx(eng_mod):
    e = context(eng_mod)
    yield e
    e.close()


def grid_reference(case):
    """(C, V0, V, hist) of the restatement: computed once per case, shared and never written to (the cases of 4095 and 4096, 134 MB
    each and used once, are not kept)."""
    return _kept(case) if case[1] <= 2049 else _reference(case)


def _reference(case):
    name, N, T, seed = case
    C, V0 = mc.problem(name, N, seed)
    V, hist, sweeps = mc.mixing_reference(C, V0, T, 0.0)
    assert sweeps == T
    for a in (C, V0, V, hist):
        a.setflags(write=False)
    return C, V0, V, hist


_kept = functools.lru_cache(maxsize=None)(_reference)


@functools.lru_cache(maxsize=None)
def stop_reference(case):
    name, N, tol, seed = case
    C, V0 = mc.problem(name, N, seed)
    V, hist, sweeps = mc.mixing_reference(C, V0, mc.STOP_MAX_SWEEPS, tol)
    for a in (C, V0, V, hist):
        a.setflags(write=False)
    return C, V0, V, hist, sweeps


def case_of(name, N):
    return [c for c in mc.grid() if c[:2] == (name, N)][0]


def check_grid_case(e, case):
    C, V0, Vr, hr = grid_reference(case)
    name, N, T, _ = case
    V, hist, sweeps = e.sdr_solve_unitdiag(C, V0=V0, max_sweeps=T, tol=0.0)
    assert sweeps == T and hist.size == T + 2, (case, sweeps, hist.size)
    dv = float(np.max(np.abs(V - Vr)))
    dh = float(np.max(np.abs(hist - hr) / (1.0 + np.abs(hr))))
    dt = abs(hist[T] - hist[T + 1]) / (1.0 + abs(hist[T + 1]))
    stay = mc.zero_g_rows(C)
    moved = np.setdiff1d(np.arange(N), stay)
    dn = float(np.max(np.abs(np.linalg.norm(V[moved], axis=1) - 1.0)))
    print('%s: max |V - V_ref| %.3e, max |hist - hist_ref| / (1 + |hist_ref|) %.3e, tracked against recomputed %.3e, '
          'max | |v_i| - 1 | %.3e' % (mc.grid_id(case), dv, dh, dt, dn))
    assert dv <= 1e-12, (case, dv)
    assert dh <= 1e-12, (case, dh, hist, hr)
    assert dt <= 1e-12, (case, hist)
    assert dn <= 1e-14, (case, dn)
    assert stay.size == (2 if name == 'cut' else 0)
    assert np.array_equal(V[stay], V0[stay]), case
    return dv, dh


@pytest.mark.parametrize('case', mc.grid(), ids=mc.grid_id)
def test_the_kernel_follows_the_restatement(ctx, case):
    check_grid_case(ctx, case)


@pytest.mark.parametrize('case', mc.stop_cases(), ids=mc.stop_id)
def test_stop_rule_and_jump_to_the_last_pass(ctx, case):
    """max_sweeps far above the stop: the sweep count is the restatement's, hist[sweeps + 1] is the value recomputed from the returned
    V, and the history beyond it is left alone -- seen through the raw entry with a buffer of sentinels: the entry copies its
    max_sweeps + 2 entries back (the kernel's buffer, cleared before the launch) and nothing past them."""
    from qcqp_amd.engine import _dp
    C, V0, Vr, hr, sr = stop_reference(case)
    tol, M = case[2], mc.STOP_MAX_SWEEPS
    V, hist, sweeps = ctx.sdr_solve_unitdiag(C, V0=V0, max_sweeps=M, tol=tol)
    print('%s: %d sweeps (restatement %d), max |V - V_ref| %.3e' % (mc.stop_id(case), sweeps, sr, np.max(np.abs(V - Vr))))
    assert sweeps == sr and hist.size == sr + 2, (case, sweeps, sr)
    assert np.max(np.abs(V - Vr)) <= 1e-12, case
    assert np.max(np.abs(hist - hr) / (1.0 + np.abs(hr))) <= 1e-12, case
    f = mc.objective(C, V)
    assert abs(hist[sweeps + 1] - f) <= 1e-12 * (1.0 + abs(f)), (case, hist[sweeps + 1], f)
    raw = np.full(M + 2 + 16, SENTINEL)
    Vraw = V0.copy()
    sw = ctypes.c_int(-5)
    assert ctx.L.qcqpmi_sdr_solve_unitdiag(ctx.h, _dp(C), C.shape[0], _dp(Vraw), M, tol, _dp(raw), ctypes.byref(sw)) == 0
    assert sw.value == sweeps and np.array_equal(Vraw, V) and np.array_equal(raw[:sweeps + 2], hist)
    rest = raw[sweeps + 2:M + 2]
    assert np.all(rest == 0.0) or np.all(rest == SENTINEL), (case, rest[:4])
    assert np.all(raw[M + 2:] == SENTINEL)


@pytest.mark.parametrize('N', [3, 257])
def test_no_sweeps(ctx, N):
    """max_sweeps = 0: the start comes back bit for bit, and both history entries are the objective of the start -- bit-equal to each
    other, because both objective passes add the same numbers in the same order whatever the parity of the row buffers."""
    C, V0, _, _ = grid_reference(case_of('dense', N))
    V, hist, sweeps = ctx.sdr_solve_unitdiag(C, V0=V0, max_sweeps=0, tol=0.0)
    assert sweeps == 0 and hist.size == 2 and np.array_equal(V, V0)
    assert hist[0] == hist[1], hist
    f = mc.objective(C, V0)
    assert abs(hist[0] - f) <= 1e-12 * (1.0 + abs(f)), (hist, f)


def test_a_cost_that_moves_no_row(ctx):
    """Only the diagonal is nonzero: every g_i is zero, every row stays, dsweep is exactly zero and the first sweep is the last even
    with tol = 0."""
    C, V0 = mc.zero_cost_case()
    V, hist, sweeps = ctx.sdr_solve_unitdiag(C, V0=V0, max_sweeps=5, tol=0.0)
    Vr, hr, sr = mc.mixing_reference(C, V0, 5, 0.0)
    assert sweeps == sr == 1 and hist.size == 3 and np.array_equal(V, V0)
    assert np.max(np.abs(hist - hr)) <= 1e-12 * (1.0 + np.trace(C)) and hist[0] == hist[1] == hist[2]


@pytest.mark.parametrize('N,other', [(321, 2049), (2049, 65)])
def test_bit_for_bit_across_calls_and_contexts(eng_mod, ctx, N, other):
    case = case_of('dense', N)
    C, V0, _, _ = grid_reference(case)
    Co, V0o, _, _ = grid_reference(case_of('dense', other))
    a = ctx.sdr_solve_unitdiag(C, V0=V0, max_sweeps=case[2], tol=0.0)
    ctx.sdr_solve_unitdiag(Co, V0=V0o, max_sweeps=2, tol=0.0)
    b = ctx.sdr_solve_unitdiag(C, V0=V0, max_sweeps=case[2], tol=0.0)
    fresh = context(eng_mod)
    c = fresh.sdr_solve_unitdiag(C, V0=V0, max_sweeps=case[2], tol=0.0)
    fresh.close()
    for o in (b, c):
        assert np.array_equal(a[0], o[0]) and np.array_equal(a[1], o[1]) and a[2] == o[2]


def rounding(C, y):
    """N^2 eps (max |y| + N max |C|): what bound and primal carry from their own evaluation (tests/test_gpu_sdr_batch.py)."""
    N = C.shape[0]
    return N * N * EPS * (np.max(np.abs(y)) + N * np.max(np.abs(C)))


def converged_problem(name):
    from qcqp_amd import problems
    if name == 'bls':       # 512 rows, seed 2: 628 sweeps in the restatement, lambda_min / scale -1.1e-08
        return problems.boolean_least_squares(256, 512, seed=2)[0]
    return problems.maxcut(300, seed=1)[0]      # 725 sweeps, lambda_min / scale -8e-11


@pytest.mark.parametrize('name', ['bls', 'maxcut'])
def test_to_convergence_beyond_65(eng_mod, name):
    """solve_sdr with its own limits (5000 sweeps, tol = 1e-11) at N = 257 and N = 301: certified, monotone, diag(X) = d, and the
    primal value of the restatement run to the same tolerance from the same start (seed 0 as Engine.sdr_solve_unitdiag draws it)
    -- within the larger of the two certified gaps, as sweep counts to 1e-11 may differ by a few."""
    from qcqp_amd import sdr
    from qcqp_amd.form import QCQPForm
    form = QCQPForm.from_arrays(converged_problem(name))
    e = eng_mod.Engine(form)
    X, bound, info = sdr.solve_sdr(e, form)
    e.close()
    C, V, hist = info['C'], info['V'], info['hist']
    N = C.shape[0]
    scale = 1.0 + np.max(np.abs(C))
    assert info['converged'] and not info['sweep_limit_hit'] and 0 < info['sweeps'] < 5000, info['sweeps']
    assert info['lambda_min'] >= -1e-6 * scale, (info['lambda_min'], scale)
    p1 = info['primal']
    assert bound == info['dual_bound'] and bound <= p1, (bound, p1)
    assert np.all(np.diff(hist[:-1]) <= 1e-9), np.max(np.diff(hist[:-1]))
    assert np.max(np.abs(np.diag(X) - 1.0)) <= 1e-12                     # d = 1 in both problems
    V0 = np.random.RandomState(0).randn(N, mc.K)
    V0 /= np.linalg.norm(V0, axis=1)[:, None]
    Vr, hr, sr = mc.mixing_reference(C, V0, 5000, 1e-11)
    y2, lmin2, bound2 = sdr.dual_certificate(C, Vr)
    p2 = float(hr[-1])
    rnd = max(rounding(C, info['y']), rounding(C, y2))
    print('%s: sweeps %d / %d, primal %.15g / %.15g, gaps %.3e / %.3e, lambda_min / scale %.3e'
          % (name, info['sweeps'], sr, p1, p2, p1 - bound, p2 - bound2, info['lambda_min'] / scale))
    assert sr < 5000 and lmin2 >= -1e-6 * scale
    assert abs(p1 - p2) <= max(p1 - bound, p2 - bound2) + rnd, (p1, p2, bound, bound2)


def test_refusals_and_a_solve_after_them(eng_mod):
    e = context(eng_mod)

    def refused(code, C, **kw):
        with pytest.raises(eng_mod.EngineError) as ex:
            e.sdr_solve_unitdiag(C, **kw)
        assert ex.value.code == code, (ex.value.code, str(ex.value))

    C, V0, _, _ = grid_reference(case_of('dense', 65))
    refused(-1, np.ones((1, 1)), V0=np.ones((1, 64)) / 8.0)             # N = 1: QCQPMI_EINVAL
    # N = 4097: QCQPMI_EUNSUPPORTED, refused before anything is copied (np.zeros: pages that are never touched)
    refused(-4, np.zeros((4097, 4097)), V0=np.zeros((4097, 64)))
    refused(-1, C, V0=V0, max_sweeps=-1)
    refused(-1, C, V0=V0, tol=float('nan'))
    refused(-1, C, V0=V0, tol=-1.0)
    check_grid_case(e, case_of('dense', 65))
    check_grid_case(e, case_of('cut', 257))
    e.close()
