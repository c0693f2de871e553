"""What tests/test_admm_setup_cpu.py, tests/test_setup_grid_cpu.py and tests/test_gpu_admm_setup.py share (a plain module, no test in it).

restate            admm_setup_kernel / admm_setup_wide_kernel in NumPy (csrc/admm_setup.h), built from the restatements of the two
                   eigen-solvers that the project already has -- spectral_batch_cases.jacobi for n <= 64, spectral_wide_cases.jacobi_wide
                   plus Rayleigh quotients past it -- and adding what is new: the rho rule in the kernel's order of operations, the test
                   of a given rho, the weights w_k and Minv_b = sum_k (u_k u_k') w_k over k in the solver's order.  NumPy has no fma: a
                   sum differs from the kernel's in its last bits.
family             the families of the grid: bls (lambda_min > 0), cut (< 0), box (indefinite diagonal) of admm_batch_cases, and three
                   added here over Boolean constraints -- ident (P0 = I), zero (P0 = 0: lambda_min exactly 0, the 50 / m branch, and
                   |P0|_F == 0 is the wide solver's special case), diag (a diagonal P0 of mixed sign: the solvers find its eigenvalues
                   exactly, so rho is the host's bit for bit).
LMIN_BOUND         the GPU test's bound on |lambda_min - eigvalsh| / |P0_b|_F, with the measurement it comes from.
"""
import functools

import numpy as np

import admm_batch_cases as ab
import spectral_batch_cases as sc
import spectral_wide_cases as wc

SIZES = (1, 2, 3, 31, 32, 33, 63, 64)
SIZES_WIDE = (65, 66, 95, 96, 127, 128)
BS = (1, 3)
FAMILIES = ('bls', 'cut', 'box', 'ident', 'zero', 'diag')
SEED = 9
MAX_SWEEPS, TOL = sc.MAX_SWEEPS, sc.TOL
RHO_RTOL = 1e-12             # the project's own: tests/test_admm_batch_cpu.py::test_rho_rule_and_batched_inverse_agree_with_the_oracle
SOLVE_RTOL = 1e-12           # likewise, for ab.rel(Minv_b rhs, z) against the oracle's Cholesky solve
LMIN_GATE = 1e-8             # rho is compared with the host's only where |lambda_min| > LMIN_GATE |P0_b|_F: the rule jumps at 0
# |lambda_min - eigvalsh(P0_b)[0]| / |P0_b|_F of the NumPy restatement over the whole grid (FAMILIES x SIZES + SIZES_WIDE, the three
# problems of B = 3): the worst is LMIN_MEASURED (tests/test_setup_grid_cpu.py asserts that it is not exceeded).  The GPU test allows
# ten times that: the kernels sum in other, fixed orders (fma, ascending index) than NumPy's pairwise sums.
LMIN_MEASURED = 7.8e-16      # measured 7.74e-16; rho then within 1.8e-15 of auto_rho(), Minv within 7.9e-14 of admm_minvs'
LMIN_BOUND = 10.0 * LMIN_MEASURED


def family(name, n, B, seed=SEED):
    """B problems (funcs lists, objective first) over shared separable constraints; problem b depends on (name, n, seed + b) alone."""
    if name in ('bls', 'cut', 'box'):
        return ab.family(name, n, B, seed=seed)
    cons = ab.family('bls', n, 1, seed=seed)[0][1:]
    out = []
    for b in range(B):
        if name == 'ident':
            P0 = np.eye(n)
        elif name == 'zero':
            P0 = np.zeros((n, n))
        elif name == 'diag':          # mixed sign, magnitudes over three decades, at least one negative entry
            rs = np.random.RandomState(1000 * n + seed + b)
            d = rs.randn(n) * 10.0 ** rs.uniform(-1.5, 1.5, size=n)
            d[rs.randint(n)] = -abs(rs.randn()) - 0.5
            P0 = np.diag(d)
        else:
            raise KeyError(name)
        q0 = np.random.RandomState(77 + seed + b).randn(n)
        out.append([(P0, q0, 0.25 * b, None)] + cons)
    return out


def cases():
    """(family, n, B) over both widths."""
    return [(name, n, B) for name in FAMILIES for n in SIZES + SIZES_WIDE for B in BS]


def case_id(c):
    return '%s-n%d-B%d' % c


def rho_rule(lmin, m):
    """admm_setup_rho of csrc/admm_setup_rule.h -- admm_rhos' expression, one problem."""
    m = float(m)
    return 50.0 * ((2.0 * (1.0 - lmin)) / m) if lmin < 0.0 else 50.0 * (1.0 / m)


def restate(P0, m, rho=None, max_sweeps=MAX_SWEEPS, tol=TOL):
    """One problem as the setup kernels solve it: dict(rho, lambda_min, Minv, sweeps, status, lam, U) -- U with COLUMN k = u_k, lam in
    the solver's order.  Minv is None where status == 3."""
    P0 = np.asarray(P0, dtype=np.float64)
    n, m = P0.shape[0], float(m)
    if n <= 64:
        lam, Q, sweeps, conv = sc.jacobi(P0, max_sweeps, tol)
        U = np.ascontiguousarray(Q.T)
    else:
        U2, sweeps, conv, _ = wc.jacobi_wide(P0, max_sweeps, tol)
        U = np.ascontiguousarray(U2[:n, :n])      # the padding coordinate of an odd n is the unit column n2 - 1: left out
        lam = np.einsum('ik,ik->k', U, P0.dot(U))
    lmin = float(np.min(lam))
    given = rho is not None
    rho_b = float(rho) if given else rho_rule(lmin, m)
    out = dict(rho=rho_b, lambda_min=lmin, sweeps=sweeps, lam=lam, U=U, Minv=None)
    if given and lmin + m * rho_b < 0.0:
        out['status'] = 3
        return out
    with np.errstate(divide='ignore'):
        w = 1.0 / (2.0 * (lam + rho_b * m))
    Minv = np.zeros((n, n))
    for k in range(n):
        Minv = Minv + (U[:, k][:, None] * U[:, k][None, :]) * w[k]
    out['Minv'] = Minv
    finite = np.isfinite(lmin) and np.isfinite(rho_b) and np.all(np.isfinite(w)) and np.all(np.isfinite(Minv))
    finite = finite and not (sc.degenerate_norm(P0) if n <= 64 else wc.degenerate_norm(P0))      # (the solvers' `degenerate`: status 2)
    out['status'] = 0 if (finite and conv) else (2 if not finite else 1)
    return out


@functools.lru_cache(maxsize=None)
def problem(name, n, b):
    """(funcs, P0, m) of problem b of the family at the grid's seed."""
    funcs = family(name, n, b + 1)[b]
    return funcs, np.ascontiguousarray(sc.objectives([funcs])[0][0]), len(funcs) - 1


@functools.lru_cache(maxsize=None)
def restated(name, n, b):
    """The restatement of problem b of the family, rho by the rule (one computation, shared by the tests; treat it as read-only)."""
    _, P0, m = problem(name, n, b)
    return restate(P0, m)


def cholesky_solve(P0, rho, m, rhs):
    """The oracle's z-update solve: Cholesky of 2 (P0 + rho m I), forward and back substitution."""
    L = np.linalg.cholesky(2.0 * (P0 + rho * m * np.eye(P0.shape[0])))
    return np.linalg.solve(L.T, np.linalg.solve(L, rhs))


def given_rho_case(n=16):
    """The batch of tests/test_admm_batch_cpu.py's given-rho check -- cut, n = 16, B = 3, seed 2; or the same at another n -- with a rho that is large enough
    for every problem and one that is too small for some and large enough for the others, in the middle (geometric) of the widest
    gap between two of the thresholds -lambda_min / m and so at least 1 % away from every one of them:
    (funcs list, P0s, m, rho_ok, rho_small, lmin by eigvalsh)."""
    fl = ab.family('cut', n, 3, seed=2)
    P0s = sc.objectives(fl)[0]
    m = len(fl[0]) - 1
    lmin = np.linalg.eigvalsh(P0s)[:, 0]
    assert np.all(lmin < 0)
    thr = np.sort(-lmin / m)
    g = int(np.argmax(thr[1:] / thr[:-1]))
    assert thr[g + 1] / thr[g] > 1.01 ** 2
    return fl, P0s, m, float(thr[-1] * 1.01), float(np.sqrt(thr[g] * thr[g + 1])), lmin
