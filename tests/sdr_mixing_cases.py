"""What tests/test_sdr_mixing_cpu.py and tests/test_gpu_sdr_mixing.py share: a plain restatement of sdr_mixing_kernel's passes
(csrc/sdr_solve.h, qcqpmi_sdr_solve_unitdiag) for ONE problem, sweep by sweep and with the kernel's meaning of the history, and the
grid of its domain -- families of C, sizes N = 2 .. 4096 around every size at which the kernel takes another path (register slots of
64 columns, groups of four slots = 256 columns, odd / even N for the swap of the row buffers, the 64 KB LDS image), the stop-rule
cases and their margin.  A plain module, not a conftest: the test files import what they use."""
import numpy as np

import sdr_batch_cases as sc

K = sc.K
NS = (2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320, 321, 513, 1025, 2049)
FAMILIES = ('dense', 'bls', 'cut')
CUT_FROM = 63        # below, the isolated vertex leaves a graph without edges: every g_i is zero and tol = 0 stops after one sweep
                     # (that corner is a test of its own, see zero_cost_case)
LONGDOUBLE_UPTO = 513
STOP_MAX_SWEEPS = 400
MARGIN = 1e-6


def sweeps_of(N):
    """T of the grid: 3 sweeps, 2 above N = 1025.  N = 2 is at its fixed point after ONE sweep (v_0 <- -+v_1, v_1 <- -+v_0): the
    dsweep of a second sweep is rounding noise or exactly zero, and with tol = 0 an exact zero stops the run -- the sweep count
    would hinge on a last bit, so N = 2 runs one sweep."""
    return 1 if N == 2 else 2 if N > 1025 else 3


def unit_rows(N, seed):
    V0 = np.random.RandomState(seed).randn(N, K)
    V0 /= np.linalg.norm(V0, axis=1)[:, None]
    return V0


def cost(name, N, seed):
    """C (N, N) symmetric of the family.  dense: Gaussian, nonzero diagonal.  bls: sdr.lifted_cost of Boolean least squares in
    n = N - 1 variables (large positive entries, C[n, n] = r0, last row and column q0 / 2).  cut: the lifted weighted MAXCUT of
    sdr_batch_cases.family('cut', ...) with vertex n // 2 isolated -- rows n // 2 and n (q0 = 0) have g_i = 0 exactly."""
    n = N - 1
    if name == 'dense':
        A = np.random.RandomState(seed).randn(N, N)
        return (A + A.T) / np.sqrt(2.0)
    if name == 'bls':
        from qcqp_amd import problems, sdr
        from qcqp_amd.form import QCQPForm
        funcs = problems.boolean_least_squares(n, n + n // 2 + 1, seed=seed)[0]
        form = QCQPForm.from_arrays(funcs[:1])      # the objective alone: lifted_cost reads nothing else, d = 1 (x_i^2 == 1)
        return sdr.lifted_cost(form, np.ones(n))[0]
    if name == 'cut':
        from qcqp_amd import problems       # the one problem of sc.family('cut', n, 1, seed) without building its constraints twice
        P0, q0, r0, _ = problems.maxcut(n, seed=seed, weighted=True)[0][0]
        C = sc.lifted(np.asarray(P0)[None], q0[None], np.array([r0]), np.ones(n))[0]
        C[n // 2, :] = 0.0
        C[:, n // 2] = 0.0
        return C
    raise KeyError(name)


def zero_g_rows(C):
    """The rows whose off-diagonal part is zero: g_i = 0 exactly on every pass, the row stays as it is."""
    off = C - np.diag(np.diag(C))
    return np.nonzero(~off.any(axis=1))[0]


def grid():
    """(family, N, T, seed): every N with dense and bls, cut from N = 63, dense alone at 4095, dense and cut at 4096."""
    out = []
    for j, N in enumerate(NS):
        for k0, name in enumerate(FAMILIES):
            if name == 'cut' and N < CUT_FROM:
                continue
            out.append((name, N, sweeps_of(N), 7 + j + 100 * k0))
    out.append(('dense', 4095, 2, 31))
    out.append(('dense', 4096, 2, 32))
    out.append(('cut', 4096, 2, 232))
    return out


def grid_id(c):
    return '%s-N%d' % c[:2]


def stop_cases():
    """(family, N, tol, seed): the stop rule decides the sweep count; tests/test_sdr_mixing_cpu.py holds every one of them to the
    margin condition (stop_margin), so the count cannot hinge on a last-bit difference."""
    return [(name, N, tol, 41 + N + (0 if name == 'dense' else 100))
            for name in ('dense', 'bls') for N in (129, 257) for tol in (1e-2, 1e-4)]


def stop_id(c):
    return '%s-N%d-tol%g' % c[:3]


def problem(name, N, seed):
    """(C, V0) of a case: the start draws from its own RandomState."""
    return cost(name, N, seed), unit_rows(N, 1000 + seed)


def zero_cost_case(N=65):
    """C = 0 but for its diagonal: every g_i is zero, no row moves, dsweep = 0 and tol = 0 stops after the first sweep."""
    return np.diag(np.arange(1.0, N + 1.0)), unit_rows(N, 5)


def objective(C, V):
    return float(((C @ V) * V).sum())


def mixing_reference(C, V0, max_sweeps, tol, dtype=np.float64, ratios=None):
    """sdr_mixing_kernel restated for one problem.  Pass -1: hist[0] = sum_i (v_i . g_i + C_ii), g_i = sum_{j != i} C_ij v_j (unit
    rows).  Update sweeps: cyclic v_i <- -g_i / |g_i| (a row with |g_i| == 0 stays as it is), the objective tracked by the exact
    change -2 (|g_i| + g_i . v_i) of every update, hist[t] after sweep t; stop at |dsweep| <= tol (1 + |f|) or max_sweeps.  Last
    pass: hist[sweeps + 1] recomputed from scratch.  Returns (V, hist, sweeps), hist of sweeps + 2 entries.  ratios: a list that
    receives |dsweep| / (tol (1 + |f|)) of every sweep (tol > 0)."""
    C = np.asarray(C, dtype=dtype)
    V = np.array(V0, dtype=dtype)
    N = C.shape[0]
    dg = np.diag(C).copy()
    two = dtype(2.0)

    def from_scratch():
        G = C @ V - dg[:, None] * V
        return ((G * V).sum(axis=1) + dg).sum()

    f = from_scratch()
    hist = [f]
    sweeps = 0
    while sweeps < max_sweeps:
        dsweep = dtype(0.0)
        for i in range(N):
            g = C[i] @ V - dg[i] * V[i]
            nrm = np.sqrt(g @ g)
            if nrm > 0.0:
                dsweep += -two * (nrm + g @ V[i])
                V[i] = -g / nrm
        f = f + dsweep
        sweeps += 1
        hist.append(f)
        bound = tol * (1.0 + abs(f))
        if ratios is not None and tol > 0.0:
            ratios.append(float(abs(dsweep) / bound))
        if abs(dsweep) <= bound:
            break
    hist.append(from_scratch())
    return V, np.array(hist, dtype=dtype), sweeps


def stop_margin(ratios):
    """True if no sweep's |dsweep| / (tol (1 + |f|)) lies in [1 - MARGIN, 1 + MARGIN]."""
    r = np.asarray(ratios)
    return bool(np.all((r < 1.0 - MARGIN) | (r > 1.0 + MARGIN)))
