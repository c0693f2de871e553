"""The yardstick of tests/test_gpu_sdr_mixing.py without a GPU: sdr_mixing_cases.mixing_reference -- sdr_mixing_kernel's passes
(csrc/sdr_solve.h) restated for one problem -- is held to a long double run of itself on every grid case with N <= 513 (1e-13 in V,
1e-13 (1 + |f|) in every history entry; measured: 8.0e-16 and 1.1e-14), to sdr_batch_cases.mixing_numpy on the stop-rule cases (final V
and sweep count), and to the properties of the method: the history does not increase over the update sweeps, the tracked and the
recomputed last value agree, the two rows of the MAXCUT family whose g is zero come back bit-equal to their start.  Every committed
stop-rule case keeps |dsweep| / (tol (1 + |f|)) outside [1 - 1e-6, 1 + 1e-6] on every sweep it runs, so the sweep count the GPU file
asserts cannot hinge on a last-bit difference.  90 tests, about 7 s, most of it long double products."""
import functools

import numpy as np
import pytest

import sdr_mixing_cases as mc
import sdr_batch_cases as sc

SMALL = [c for c in mc.grid() if c[1] <= mc.LONGDOUBLE_UPTO]


@functools.lru_cache(maxsize=None)
def reference(case):
    name, N, T, seed = case
    C, V0 = mc.problem(name, N, seed)
    return (C, V0) + mc.mixing_reference(C, V0, T, 0.0)


@functools.lru_cache(maxsize=None)
def stopped(case):
    name, N, tol, seed = case
    C, V0 = mc.problem(name, N, seed)
    ratios = []
    return (C, V0) + mc.mixing_reference(C, V0, mc.STOP_MAX_SWEEPS, tol, ratios=ratios) + (ratios,)


def test_the_grid_is_the_documented_one():
    g = mc.grid()
    assert len(set(g)) == len(g) == 49
    for N in mc.NS:
        assert sum(1 for c in g if c[1] == N) >= 2, N
    assert [c[0] for c in g if c[1] == 4095] == ['dense'] and sorted(c[0] for c in g if c[1] == 4096) == ['cut', 'dense']
    assert all(c[2] == (1 if c[1] == 2 else 2 if c[1] > 1025 else 3) for c in g)
    assert len(mc.stop_cases()) == 8
    # cut is the lifted problem of sdr_batch_cases.family('cut', ...) but for the isolated vertex
    fl = sc.family('cut', 64, 1, seed=9)
    ref = sc.lifted(*sc.objectives(fl), d=np.ones(64))[0]
    ref[32, :] = ref[:, 32] = 0.0
    assert np.array_equal(mc.cost('cut', 65, 9), ref)


@pytest.mark.parametrize('case', SMALL, ids=mc.grid_id)
def test_float64_against_long_double(case):
    C, V0, V, hist, sweeps = reference(case)
    T = case[2]
    Vl, histl, sweepsl = mc.mixing_reference(C, V0, T, 0.0, dtype=np.longdouble)
    assert Vl.dtype == np.longdouble and histl.dtype == np.longdouble
    assert sweeps == sweepsl == T and hist.size == histl.size == T + 2
    dv = float(np.max(np.abs(V - Vl)))
    dh = float(np.max(np.abs(hist - histl) / (1.0 + np.abs(histl))))
    print('%s: max |dV| %.3e, max |dhist| / (1 + |f|) %.3e' % (mc.grid_id(case), dv, dh))
    assert dv <= 1e-13 and dh <= 1e-13, (case, dv, dh)


@pytest.mark.parametrize('case', SMALL, ids=mc.grid_id)
def test_history_and_rows_of_the_restatement(case):
    C, V0, V, hist, sweeps = reference(case)
    name, N, T, _ = case
    scale = 1.0 + np.abs(hist)
    assert np.all(np.diff(hist[:T + 1]) <= 1e-12 * scale[1:T + 1]), (case, hist)
    assert abs(hist[T] - hist[T + 1]) <= 1e-12 * scale[T + 1], (case, hist)
    assert abs(hist[T + 1] - mc.objective(C, V)) <= 1e-12 * scale[T + 1]
    assert abs(hist[0] - mc.objective(C, V0)) <= 1e-12 * scale[0]
    stay = mc.zero_g_rows(C)
    if name == 'cut':
        assert list(stay) == [(N - 1) // 2, N - 1], (case, stay)
        assert np.array_equal(V[stay], V0[stay])
    else:
        assert stay.size == 0
    moved = np.setdiff1d(np.arange(N), stay)
    assert N == 2 or np.all(V[moved] != V0[moved])      # N = 2: v_1 <- -+v_0 = v_1 again
    assert np.max(np.abs(np.linalg.norm(V, axis=1) - 1.0)) <= 1e-14


@pytest.mark.parametrize('case', mc.stop_cases(), ids=mc.stop_id)
def test_stop_rule_cases_keep_their_margin_and_agree_with_mixing_numpy(case):
    C, V0, V, hist, sweeps, ratios = stopped(case)
    tol = case[2]
    print('%s: %d sweeps, last ratios %s' % (mc.stop_id(case), sweeps, ['%.4g' % r for r in ratios[-2:]]))
    assert 1 < sweeps < mc.STOP_MAX_SWEEPS // 2 and len(ratios) == sweeps and hist.size == sweeps + 2
    assert mc.stop_margin(ratios), (case, ratios)
    assert all(r > 1.0 for r in ratios[:-1]) and ratios[-1] < 1.0
    Vn, sn = sc.mixing_numpy(C[None], V0[None], tol=tol, max_sweeps=mc.STOP_MAX_SWEEPS)
    assert int(sn[0]) == sweeps, (case, sn, sweeps)
    assert np.max(np.abs(Vn[0] - V)) <= 1e-12, case
    scale = 1.0 + np.abs(hist)
    assert np.all(np.diff(hist[:sweeps + 1]) <= 1e-12 * scale[1:sweeps + 1])
    assert abs(hist[sweeps] - hist[sweeps + 1]) <= 1e-12 * scale[sweeps + 1]


def test_sweep_limits_and_rows_that_stay():
    """max_sweeps = 0 returns the start and two equal history entries; a cost without off-diagonal entries moves no row and stops
    after one sweep even with tol = 0 (dsweep is exactly zero)."""
    C, V0 = mc.problem('dense', 65, 3)
    V, hist, sweeps = mc.mixing_reference(C, V0, 0, 0.0)
    assert sweeps == 0 and hist.size == 2 and hist[0] == hist[1] and np.array_equal(V, V0)
    C, V0 = mc.zero_cost_case()
    V, hist, sweeps = mc.mixing_reference(C, V0, 5, 0.0)
    assert sweeps == 1 and hist.size == 3 and np.array_equal(V, V0)
    assert np.all(np.abs(hist - np.trace(C)) <= 1e-12 * (1.0 + np.trace(C)))
